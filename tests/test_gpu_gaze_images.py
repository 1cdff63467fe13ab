"""GPU tests of the gaze image path.  Every comparison is on bytes or on fp32 bits: eg_gaze_resize against Pillow's
own outputs (tests/golden/gaze_images.npz) with sentinels behind every image, the workspace and the store; eg_gaze_batch against
torch's ToTensor + Normalize tensors and Pillow's ImageEnhance outputs of the same fixture, and against the numpy restatement
(tests/gazeimg_ref.py, itself pinned to the fixture by tests/test_gaze_images_host.py) where the draws come from the hash;
ResidentMultimodal against the two stand-alone calls; one training step and one evaluation from the loader."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd import gaze as G  # noqa: E402
from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
from tests import gazeimg_ref as R  # noqa: E402
from tests.test_gaze_images_host import GOLD, NAMES, PAIRS, PARITY_SEED  # noqa: E402

DEV = "cuda"
SENTINEL = 0xA5
GUARD = 256             # sentinel bytes (or floats) behind every buffer
F, W = 16, 24
TABLE = R.normalise_table()


def stream():
    return torch.cuda.current_stream().cuda_stream


def same_bits(a: torch.Tensor, b) -> bool:
    b = torch.from_numpy(np.ascontiguousarray(b)) if isinstance(b, np.ndarray) else b
    return a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------
# eg_gaze_resize
# ---------------------------------------------------------------------------------------------------------------
def raw_resize(images, Fo, Wo, shapes=None):
    """one eg_gaze_resize call assembled here, with SENTINEL bytes behind every image (up to and beyond its 16-byte boundary), the
    workspace and the store; checks them and that the inputs were only read; -> store [n, Fo, Wo, 3] uint8 (host).
    shapes overrides the (h, w) tables the kernel sees (a skipped image)."""
    n = len(images)
    shapes = shapes or [im.shape[:2] for im in images]
    off, mid_off, at, mid = [], [], 0, 0
    for im in images:
        off.append(at)
        mid_off.append(mid)
        at += -(-im.size // 16) * 16 + 16
        mid += -(-(3 * Wo * im.shape[0]) // 16) * 16
    host = np.full(at + GUARD, SENTINEL, np.uint8)
    for im, o in zip(images, off):
        host[o:o + im.size] = im.reshape(-1)
    where, parts, words = {}, [], 0
    for key in [(im.shape[1], Wo) for im in images] + [(im.shape[0], Fo) for im in images]:
        if key not in where:
            where[key] = words
            parts.append(G.resize_tables(*key))
            words += parts[-1].size
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
    data, tabs = up(host, np.uint8), up(np.concatenate(parts), np.int32)
    t_off, t_mid = up(off, np.int64), up(mid_off, np.int64)
    t_h, t_w = up([s[0] for s in shapes], np.int32), up([s[1] for s in shapes], np.int32)
    t_ht, t_vt = up([where[(im.shape[1], Wo)] for im in images], np.int64), up([where[(im.shape[0], Fo)] for im in images], np.int64)
    sum_h = sum(im.shape[0] for im in images)
    need = L.gaze_resize_workspace_bytes(n, sum_h, Wo)
    assert need >= mid
    ws = torch.full((need + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    store = torch.full((n * Fo * Wo * 3 + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    desc = L.GazeResizeDesc(ptr(data), ptr(t_off), ptr(t_h), ptr(t_w), ptr(t_mid), ptr(tabs), ptr(t_ht), ptr(t_vt), sum_h, n,
                            max(im.shape[0] for im in images), Fo, Wo)
    call("eg_gaze_resize", ctypes.byref(desc), ptr(ws), need, ptr(store), stream())
    assert data.cpu().numpy().tobytes() == host.tobytes()                                          # inputs (and their gaps) are only read
    assert (ws[need:] == SENTINEL).all() and (store[n * Fo * Wo * 3:] == SENTINEL).all()
    return store[:n * Fo * Wo * 3].view(n, Fo, Wo, 3).cpu().numpy()


def inputs(names=NAMES):
    return [GOLD[f"input/{n}"] for n in names]


def test_resize_ragged_and_single_calls_give_pillows_bytes():
    want = np.stack([GOLD[f"small/{n}"] for n in NAMES])
    ragged = raw_resize(inputs(), F, W)                                                            # 3x4096, the widest row, among them
    assert np.array_equal(ragged, want)
    for i, im in enumerate(inputs()):
        assert np.array_equal(raw_resize([im], F, W)[0], want[i]), NAMES[i]
    large = [str(n) for n in GOLD["large_of"]]
    assert np.array_equal(raw_resize(inputs(large), 64, 64), np.stack([GOLD[f"large/{n}"] for n in large]))      # 16-byte rows, upscaling
    odd = ["10x7", "37x53", "5x1000", "1x1"]
    assert np.array_equal(raw_resize(inputs(odd), 9, 11), np.stack([R.resize(im, 9, 11) for im in inputs(odd)]))  # byte-wide rows


def test_resize_skips_an_image_outside_the_served_range():
    ims = inputs(["10x7", "37x53", "24x16"])
    got = raw_resize(ims, F, W, shapes=[(10, 7), (37, 0), (24, 16)])
    assert np.array_equal(got[0], GOLD["small/10x7"]) and np.array_equal(got[2], GOLD["small/24x16"])
    assert (got[1] == SENTINEL).all()


def test_store_builds_in_bounded_batches(monkeypatch):
    want = np.stack([GOLD[f"small/{n}"] for n in NAMES])
    whole = G.GazeImageStore.from_arrays(inputs(), (F, W), DEV)
    monkeypatch.setattr(G, "RESIZE_BATCH_BYTES", 40_000)                                           # several calls
    parts = G.GazeImageStore.from_arrays(inputs(), (F, W), DEV)
    assert whole.data.dtype == torch.uint8 and tuple(whole.data.shape) == (9, F, W, 3) and len(whole) == 9
    assert np.array_equal(whole.data.cpu().numpy(), want) and np.array_equal(parts.data.cpu().numpy(), want)
    assert same_bits(whole.norm, TABLE)
    square = G.GazeImageStore.from_arrays(inputs(["135x240"]), 64, DEV)
    assert np.array_equal(square.data.cpu().numpy()[0], GOLD["large/135x240"])
    with pytest.raises(ValueError, match="3x4097"):
        G.GazeImageStore.from_arrays([np.zeros((3, 4097, 3), np.uint8)], (F, W), DEV)


# ---------------------------------------------------------------------------------------------------------------
# eg_gaze_batch
# ---------------------------------------------------------------------------------------------------------------
def fixture_store():
    return G.GazeImageStore(torch.from_numpy(np.stack([GOLD[f"small/{n}"] for n in NAMES])).to(DEV))


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


PAIR_IMG = np.asarray([[0, 1], [2, 3], [4, 4], [5, 6], [7, 8], [1, 0]], np.int32)              # pair 2: both players, one image
WIN_PAIR = np.asarray([0, 0, 1, 2, 2, 3, 4, 5, 5, 1, 3, 0], np.int32)
ORDER = np.asarray([11, 4, 7, 3, 8, 4, 0, 9, 2, 6, 10], np.int32)                                 # [3:8] = windows 3, 8, 4, 0, 9: pairs 2, 5, 2, 0, 1


def raw_batch(store, first, n, rgb=True):
    """eg_gaze_batch without augmentation into guarded outputs"""
    npx = store.F * store.W
    outs = [torch.full((n * npx * (3 if k >= 2 else 1) + GUARD,), 12345.0, device=DEV) for k in range(4 if rgb else 2)]
    tabs = [dev_i32(PAIR_IMG), dev_i32(WIN_PAIR), dev_i32(ORDER)]
    call("eg_gaze_batch", ptr(store.data), store.n, store.F, store.W, ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]), len(ORDER), first, n,
         ptr(store.norm), 0, 0, 0.0, 0.0, 0.0, 0, ptr(outs[0]), ptr(outs[1]), ptr(outs[2]) if rgb else 0, ptr(outs[3]) if rgb else 0, stream())
    for o in outs:
        assert (o[-GUARD:] == 12345.0).all()
    img = [o[:-GUARD].view(n, store.F, store.W) for o in outs[:2]]
    return img + [o[:-GUARD].view(n, 3, store.F, store.W) for o in outs[2:]]


def test_batch_without_augmentation_is_totensor_normalize_mean():
    store = fixture_store()
    before = store.data.clone()
    first, n = 3, 5
    img1, img2, rgb1, rgb2 = raw_batch(store, first, n)
    for j in range(n):
        for pl, (img, rgb) in enumerate(((img1, rgb1), (img2, rgb2))):
            name = NAMES[PAIR_IMG[WIN_PAIR[ORDER[first + j]], pl]]
            assert same_bits(rgb[j], GOLD[f"rgb/{name}"]) and same_bits(img[j], GOLD[f"mean/{name}"]), (j, pl, name)
    assert same_bits(img1[0], img2[0]) and same_bits(img1[0], img1[2])                             # pair 2 at j = 0 and 2, one image for both
    only1, only2 = raw_batch(store, first, n, rgb=False)
    assert same_bits(only1, img1) and same_bits(only2, img2)
    got = store.batch(dev_i32(PAIR_IMG), dev_i32(WIN_PAIR), dev_i32(ORDER), first, n, rgb=True)
    assert all(same_bits(a, b) for a, b in zip(got, (img1, img2, rgb1, rgb2)))
    off = store.batch(dev_i32(PAIR_IMG), dev_i32(WIN_PAIR), dev_i32(ORDER), first, n, augmentation=G.GazeAugmentation(0.0, 0.0, 0.0), seed=5)
    assert same_bits(off[0], img1) and same_bits(off[1], img2)
    assert torch.equal(store.data, before)
    with pytest.raises(ValueError, match="order must be a contiguous int32 tensor"):
        store.batch(dev_i32(PAIR_IMG), dev_i32(WIN_PAIR), torch.from_numpy(ORDER.astype(np.int64)).to(DEV), first, n)


def test_batch_jitter_at_given_factors_is_pillows():
    store = fixture_store()
    combos = [(k, i, bc) for k in range(len(NAMES)) for i in range(len(PAIRS)) for bc in (True, False)]      # 90 images: 45 samples
    n = len(combos) // 2
    factors = np.asarray([[float(q % 3 == 0), PAIRS[i][0], PAIRS[i][1], float(bc)] for q, (k, i, bc) in enumerate(combos)], np.float32)
    pair_img = np.asarray([[combos[2 * j][0], combos[2 * j + 1][0]] for j in range(n)], np.int32)
    ids = dev_i32(np.arange(n))
    img1, img2, rgb1, rgb2 = store.batch(dev_i32(pair_img), ids, ids, 0, n, rgb=True, _factors=torch.from_numpy(factors).to(DEV))
    for q, (k, i, bc) in enumerate(combos):
        px = GOLD[f"jitter/{NAMES[k]}/{i}/{'bc' if bc else 'cb'}"]
        want_rgb, want_img = R.to_tensors(px[:, ::-1] if q % 3 == 0 else px, TABLE)
        rgb, img = ((rgb1, img1), (rgb2, img2))[q % 2]
        assert same_bits(rgb[q // 2], want_rgb) and same_bits(img[q // 2], want_img), (NAMES[k], PAIRS[i], bc)


def test_batch_augmentation_draws_are_the_restatements():
    store = fixture_store()
    host = store.data.cpu().numpy()
    rng = np.random.default_rng(11)
    pair_img = rng.integers(0, 9, (20, 2)).astype(np.int32)
    win_pair = rng.integers(0, 20, 90).astype(np.int32)
    order = rng.permutation(90).astype(np.int32)[:70]
    n, aug = 64, G.GazeAugmentation()
    flip, fb, fc, bfirst = R.draws(PARITY_SEED, np.arange(2 * n), aug.hflip_prob, aug.brightness, aug.contrast)
    assert min(int(flip.sum()), int((~flip).sum()), int(bfirst.sum()), int((~bfirst).sum())) >= 16
    tabs = (dev_i32(pair_img), dev_i32(win_pair), dev_i32(order))
    got = store.batch(*tabs, 0, n, aug, PARITY_SEED, rgb=True)
    want = R.batch(host, pair_img, win_pair, order, 0, n, TABLE, PARITY_SEED, aug.hflip_prob, aug.brightness, aug.contrast)
    assert all(same_bits(a, b) for a, b in zip(got, want))
    again = store.batch(*tabs, 0, n, aug, PARITY_SEED, rgb=True)
    assert all(same_bits(a, b) for a, b in zip(got, again))
    other = store.batch(*tabs, 0, n, aug, PARITY_SEED + 1)
    assert not same_bits(other[0], got[0]) and not same_bits(other[1], got[1])
    high = store.batch(*tabs, 0, n, aug, PARITY_SEED + (1 << 32))                                 # the seed's upper half travels too
    assert not same_bits(high[0], got[0])
    head, tail = store.batch(*tabs, 0, 40, aug, PARITY_SEED), store.batch(*tabs, 40, 24, aug, PARITY_SEED)      # the counter is first + j
    assert same_bits(torch.cat([head[0], tail[0]]), got[0]) and same_bits(torch.cat([head[1], tail[1]]), got[1])
    shifted = store.batch(*tabs, 6, 64, aug, PARITY_SEED, rgb=True)
    want = R.batch(host, pair_img, win_pair, order, 6, 64, TABLE, PARITY_SEED, aug.hflip_prob, aug.brightness, aug.contrast)
    assert all(same_bits(a, b) for a, b in zip(shifted, want))
    for only in (G.GazeAugmentation(0.0, 0.2, 0.0), G.GazeAugmentation(0.0, 0.0, 0.3), G.GazeAugmentation(1.0, 0.0, 0.0)):
        got = store.batch(*tabs, 3, 9, only, 77, rgb=True)
        want = R.batch(host, pair_img, win_pair, order, 3, 9, TABLE, 77, only.hflip_prob, only.brightness, only.contrast)
        assert all(same_bits(a, b) for a, b in zip(got, want)), only


def test_batch_on_rows_that_are_no_multiple_of_four():
    ims = inputs(["10x7", "37x53", "300x17", "135x240"])
    store = G.GazeImageStore.from_arrays(ims, (9, 11), DEV)
    host = np.stack([R.resize(im, 9, 11) for im in ims])
    assert np.array_equal(store.data.cpu().numpy(), host)
    pair_img, ids = np.asarray([[0, 1], [2, 3], [3, 0]], np.int32), np.asarray([0, 1, 2, 1, 0], np.int32)
    tabs = (dev_i32(pair_img), dev_i32(ids), dev_i32(np.arange(5)))
    for aug, seed in ((None, 0), (G.GazeAugmentation(), PARITY_SEED)):
        got = store.batch(*tabs, 0, 5, aug, seed, rgb=True)
        a = aug or G.GazeAugmentation(0.0, 0.0, 0.0)
        want = R.batch(host, pair_img, ids, np.arange(5), 0, 5, TABLE, seed, a.hflip_prob, a.brightness, a.contrast)
        assert all(same_bits(x, y) for x, y in zip(got, want))


# ---------------------------------------------------------------------------------------------------------------
# the loader
# ---------------------------------------------------------------------------------------------------------------
def recording_store(tmp_path, C, T, stride, lengths, seed):
    from eyegaze_multimodal_amd.data import build_recording_store
    rng = np.random.default_rng(seed)
    recs = {f"r{i}": rng.normal(size=(C, n)).astype(np.float32) for i, n in enumerate(lengths)}
    items = [{"player1": f"r{2 * p}", "player2": f"r{2 * p + 1}", "class": ["Single", "Competition", "Cooperation"][p % 3]}
             for p in range(len(lengths) // 2)]
    build_recording_store(items, None, {"Single": 0, "Competition": 1, "Cooperation": 2}, tmp_path, window_size=T, stride=stride, recordings=recs)
    return tmp_path


def test_resident_multimodal_batches_are_the_two_calls(tmp_path):
    from eyegaze_multimodal_amd.data import ResidentWindows
    root = recording_store(tmp_path, 4, 64, 32, [160, 170, 200, 190, 130, 128], seed=1)            # 3 pairs: 4 + 4 + 3 windows
    images = fixture_store()
    pair_img = [[0, 1], [4, 4], [7, 2]]
    aug = G.GazeAugmentation()
    train = G.ResidentMultimodal(ResidentWindows(root, 4, DEV, shuffle=True, seed=9), images, pair_img, aug)
    val = G.ResidentMultimodal(ResidentWindows(root, 4, DEV), images, pair_img)
    assert len(train) == len(val) == 3
    epochs = []
    for epoch in (0, 1):
        train.set_epoch(epoch)
        got = list(train)
        assert [b[0].shape[0] for b in got] == [4, 4, 3]
        order = dev_i32(train.eeg._order())
        for k, (img1, img2, eeg1, eeg2, labels) in enumerate(got):
            e1, e2, lab = train.eeg.store.gather(order, 4 * k, img1.shape[0], train.eeg.mode)
            i1, i2 = images.batch(dev_i32(pair_img), train.eeg.store.win_pair, order, 4 * k, img1.shape[0], aug, G.batch_seed(9, epoch, k, 0))
            assert same_bits(img1, i1) and same_bits(img2, i2) and same_bits(eeg1, e1) and same_bits(eeg2, e2) and torch.equal(labels, lab)
            assert tuple(img1.shape) == (img1.shape[0], F, W) and img1.dtype == torch.float32
        epochs.append(got)
    plain = {}
    for img1, img2, eeg1, eeg2, labels in val:                                                     # unaugmented, in storage order
        for j in range(img1.shape[0]):
            plain[len(plain)] = (img1[j], img2[j])
    wp = val.eeg.store.win_pair.cpu().numpy()
    for w, (a, b) in plain.items():
        assert same_bits(a, GOLD[f"mean/{NAMES[pair_img[wp[w]][0]]}"]) and same_bits(b, GOLD[f"mean/{NAMES[pair_img[wp[w]][1]]}"])
    # two epochs draw anew: the same window in both epochs carries another augmentation
    o0, o1 = (np.random.default_rng(9 + e).permutation(11) for e in (0, 1))
    flat = lambda got: torch.cat([b[0] for b in got])
    a, b = flat(epochs[0])[np.argsort(o0)], flat(epochs[1])[np.argsort(o1)]
    assert not same_bits(a, b)
    with pytest.raises(ValueError, match=r"integer \[3, 2\]"):
        G.ResidentMultimodal(val.eeg, images, [[0, 1]])
    with pytest.raises(ValueError, match="of a store of 9"):
        G.ResidentMultimodal(val.eeg, images, [[0, 1], [4, 4], [7, 9]])


def test_train_step_and_evaluate_from_the_loader(tmp_path):
    from eyegaze_multimodal_amd import DualEEGTransformer
    from eyegaze_multimodal_amd.data import ResidentWindows
    from eyegaze_multimodal_amd.fuzzy_gating_fusion import FuzzyGatingFusion
    from eyegaze_multimodal_amd.image_encoder import GazeCNNEncoder
    from eyegaze_multimodal_amd.train_multimodal_fuzzy_fusion import MultimodalFusionModel, MultimodalTrainer
    root = recording_store(tmp_path, 8, 1024, 512, [1536, 1600, 1700, 1536], seed=2)               # 2 pairs: 2 + 2 windows
    images = fixture_store()
    loader = G.ResidentMultimodal(ResidentWindows(root, 4, DEV, shuffle=True, seed=3), images, [[1, 7], [4, 0]], G.GazeAugmentation())
    torch.manual_seed(3)
    eeg = DualEEGTransformer(in_channels=8, num_classes=3, max_len=256, use_spectrogram=False, use_ibs=False, use_cross_attention=True,
                             d_model=64, num_layers=2, num_heads=2, d_ff=128, compute_dtype="bf16")
    model = MultimodalFusionModel(GazeCNNEncoder(num_classes=3, d_model=64, compute_dtype="bf16"), eeg, FuzzyGatingFusion(num_classes=3))
    tr = MultimodalTrainer(model, DEV, warmup_steps=1, total_steps=4)
    batch = next(iter(loader))
    out = tr.train_step(*batch)
    assert torch.isfinite(out["loss"]).all() and tuple(out["fused_logits"].shape) == (4, 3)
    ev = tr.evaluate(G.ResidentMultimodal(ResidentWindows(root, 4, DEV), images, [[1, 7], [4, 0]]))
    assert np.isfinite(ev["loss"]) and 0.0 <= ev["accuracy"] <= 1.0
