"""CPU tests of the gaze image path: the numpy restatement (tests/gazeimg_ref.py) against Pillow's and torch's own
outputs (tests/golden/gaze_images.npz, written by tests/make_golden_gaze_images.py) byte for byte, the host tables of gaze.py
against the restatement, every refusal that is reached without a GPU, and the trainer's pair filtering and image numbering."""
import ctypes
import re

import numpy as np
import pytest
import torch

from eyegaze_multimodal_amd import _lib as L
from eyegaze_multimodal_amd import engine as E
from eyegaze_multimodal_amd import gaze as G
from tests import gazeimg_ref as R
from tests.test_capi_symbols import REPO

GOLD = np.load(REPO / "tests" / "golden" / "gaze_images.npz")
NAMES = [str(n) for n in GOLD["names"]]
PAIRS = [(np.float32(b), np.float32(c)) for b, c in GOLD["factors"]]
PARITY_SEED = 20241021          # the augmentation seed of tests/test_gpu_gaze_images.py, judged below on the restatement alone


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------
# the restatement is the libraries', byte for byte
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_pillow_and_torch(name):
    img = GOLD[f"input/{name}"]
    small = R.resize(img, 16, 24)
    assert np.array_equal(small, GOLD[f"small/{name}"])
    if name in GOLD["large_of"]:
        assert np.array_equal(R.resize(img, 64, 64), GOLD[f"large/{name}"])
    for i, (fb, fc) in enumerate(PAIRS):
        assert np.array_equal(R.jitter(small, fb, fc, True), GOLD[f"jitter/{name}/{i}/bc"]), (i, "brightness first")
        assert np.array_equal(R.jitter(small, fb, fc, False), GOLD[f"jitter/{name}/{i}/cb"]), (i, "contrast first")
    rgb, mean = R.to_tensors(small, R.normalise_table())
    assert np.array_equal(bits(rgb), bits(GOLD[f"rgb/{name}"])) and np.array_equal(bits(mean), bits(GOLD[f"mean/{name}"]))


def test_fixture_covers_what_it_claims():
    assert NAMES == ["10x7", "37x53", "24x16", "16x24", "300x17", "5x1000", "3x4096", "135x240", "1x1"]
    assert np.array_equal(GOLD["small/16x24"], GOLD["input/16x24"])                                  # identity tables
    flat = sorted({float(f) for p in GOLD["factors"] for f in p})
    assert flat == [0.8, 0.93, 1.0, 1.13, 1.1999]
    changed = sum(not np.array_equal(GOLD[f"jitter/{n}/{i}/bc"], GOLD[f"jitter/{n}/{i}/cb"]) for n in NAMES for i in range(5))
    assert changed >= 10                                                                             # the order of the two is visible


# ---------------------------------------------------------------------------------------------------------------
# host tables
# ---------------------------------------------------------------------------------------------------------------
TABLE_SIZES = [(7, 24), (53, 24), (16, 16), (24, 24), (17, 24), (300, 16), (1000, 24), (4096, 24), (4096, 8), (1, 16), (240, 64), (1920, 224),
               (9, 512), (5, 16)]


@pytest.mark.parametrize("in_size,out_size", TABLE_SIZES)
def test_resize_tables_equal_the_restatement_and_keep_their_properties(in_size, out_size):
    tab = G.resize_tables(in_size, out_size)
    assert tab.dtype == np.int32 and not tab.flags.writeable
    G.validate_resize_tables(tab, in_size, out_size)
    k, xmin, count = R.axis_tables(in_size, out_size)
    ksize = int(tab[0])
    assert ksize == k.shape[1] == 2 * int(np.ceil(max(in_size / out_size, 1.0))) + 1
    assert np.array_equal(tab[1:1 + out_size], xmin) and np.array_equal(tab[1 + out_size:1 + 2 * out_size], count)
    got = tab[1 + 2 * out_size:].reshape(out_size, ksize)
    assert np.array_equal(got, k)
    assert (xmin >= 0).all() and (count >= 1).all() and (xmin + count <= in_size).all() and (count <= ksize).all()
    assert (np.abs(got.astype(np.int64).sum(axis=1) - (1 << 22)) <= count).all()                     # each rounding moves the sum by < 1
    assert (got >= 0).all() and all((got[xx, count[xx]:] == 0).all() for xx in range(out_size))


def test_validate_resize_tables_rejects_forged_tables():
    good = G.resize_tables(53, 24)
    for at, value, match in ((1 + 23, 51, r"output 23 reads \[51, 51 \+"), (1, -1, r"output 0 reads \[-1"), (1 + 24 + 5, 9, "output 5 reads"),
                             (1 + 24 + 5, 0, "output 5 reads"), (0, 5, "ksize 5")):
        bad = good.copy()
        bad[at] = value
        with pytest.raises(ValueError, match=match):
            G.validate_resize_tables(bad, 53, 24)
    with pytest.raises(ValueError, match="too short"):
        G.validate_resize_tables(good[:20], 53, 24)
    with pytest.raises(ValueError, match="expected ksize"):
        G.validate_resize_tables(good, 106, 24)                                                      # another size's table
    with pytest.raises(ValueError, match=">= 1"):
        G.resize_tables(0, 24)


def test_normalise_table_is_totensor_then_normalize():
    tab = G.normalise_table()
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (3, 256)
    assert np.array_equal(bits(tab.numpy()), bits(R.normalise_table()))
    for name in ("37x53", "3x4096"):
        px = GOLD[f"small/{name}"]
        for c in range(3):
            assert np.array_equal(bits(tab[c].numpy()[px[..., c]]), bits(GOLD[f"rgb/{name}"][c]))
    with pytest.raises(ValueError, match="three means"):
        G.normalise_table((0.5, 0.5), (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="non-zero"):
        G.normalise_table((0.5, 0.5, 0.5), (1.0, 0.0, 1.0))


def test_sites_and_binding_match_the_header():
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "eyegaze_hip.h").read_text(), flags=re.S)
    sites = {n: int(v) for n, v in re.findall(r"#define EG_SITE_IMG_(\w+)\s+(\d+)", text)}
    assert sites == dict(FLIP=E.SITE_IMG_FLIP, BRIGHT=E.SITE_IMG_BRIGHT, CONTRAST=E.SITE_IMG_CONTRAST, ORDER=E.SITE_IMG_ORDER)
    assert sites == dict(FLIP=R.SITE_IMG_FLIP, BRIGHT=R.SITE_IMG_BRIGHT, CONTRAST=R.SITE_IMG_CONTRAST, ORDER=R.SITE_IMG_ORDER)
    assert sorted(sites.values()) == [12, 13, 14, 15]
    for name in ("eg_gaze_resize_workspace_bytes", "eg_gaze_resize", "eg_gaze_batch"):
        m = re.search(r"(?:int|int64_t)\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m and len(m.group(1).split(",")) == len(L.SIGNATURES[name]), name
    assert len(L.SIGNATURES["eg_gaze_batch"]) == 22
    for name, value in (("EG_GAZE_MAX_SIDE", G.MAX_SIDE), ("EG_GAZE_MIN_OUT", G.MIN_OUT), ("EG_GAZE_MAX_OUT", G.MAX_OUT)):
        assert int(re.search(r"#define " + name + r"\s+(\d+)", text).group(1)) == value
    assert (L.GAZE_MAX_SIDE, L.GAZE_MIN_OUT, L.GAZE_MAX_OUT) == (G.MAX_SIDE, G.MIN_OUT, G.MAX_OUT)
    assert "gazeimg.hip" in __import__("eyegaze_multimodal_amd.build", fromlist=["SOURCES"]).SOURCES
    assert L.ABI_VERSION == 5


# ---------------------------------------------------------------------------------------------------------------
# draws
# ---------------------------------------------------------------------------------------------------------------
def test_parity_seed_exercises_every_branch():
    flip, fb, fc, first = R.draws(PARITY_SEED, np.arange(128), 0.5, 0.2, 0.2)
    assert 16 <= int(flip.sum()) <= 112 and 16 <= int(first.sum()) <= 112
    assert fb.dtype == fc.dtype == np.float32 and 0.8 <= fb.min() and fb.max() < 1.2 and 0.8 <= fc.min() and fc.max() < 1.2
    assert not np.array_equal(fb, fc)
    other = R.draws(PARITY_SEED + 1, np.arange(128), 0.5, 0.2, 0.2)
    assert not np.array_equal(other[0], flip) and not np.array_equal(other[1], fb)
    never = R.draws(PARITY_SEED, np.arange(128), 0.0, 0.0, 0.0)
    assert not never[0].any() and (never[1] == 1).all() and (never[2] == 1).all()
    assert R.draws(PARITY_SEED, np.arange(128), 1.0, 0.2, 0.2)[0].all()


def test_batch_seed_is_a_fixed_function_of_its_four_arguments():
    base = G.batch_seed(42, 0, 0, 0)
    assert base == G.batch_seed(42, 0, 0, 0) and 0 <= base < 1 << 64
    seen = {G.batch_seed(s, e, b, r) for s in (42, 43) for e in range(3) for b in range(4) for r in range(2)}
    assert len(seen) == 2 * 3 * 4 * 2


# ---------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------
def test_gaze_augmentation_refuses_bad_ranges():
    a = G.GazeAugmentation()
    assert (a.hflip_prob, a.brightness, a.contrast) == (0.5, 0.2, 0.2) and a.enabled
    assert not G.GazeAugmentation(0.0, 0.0, 0.0).enabled and G.GazeAugmentation(1.0, 0.0, 0.0).enabled
    for kw, match in ((dict(hflip_prob=1.5), r"hflip_prob must lie in \[0, 1\]"), (dict(hflip_prob=-0.1), "hflip_prob"),
                      (dict(brightness=1.0), r"brightness must lie in \[0, 1\)"), (dict(contrast=-0.2), r"contrast must lie in \[0, 1\)"),
                      (dict(contrast=float("nan")), "finite"), (dict(brightness=float("inf")), "finite"), (dict(hflip_prob="0.5"), "finite number"),
                      (dict(brightness=True), "finite number")):
        with pytest.raises(ValueError, match=match):
            G.GazeAugmentation(**kw)


def test_image_augmentation_yaml_form():
    import yaml
    cfg = yaml.safe_load("training:\n  epochs: 1\n  image_augmentation:\n    hflip_prob: 0.25\n    brightness: 0.1\n    contrast: 0.3\n")
    assert G.GazeAugmentation.from_config(cfg) == G.GazeAugmentation(0.25, 0.1, 0.3)
    assert G.GazeAugmentation.from_config({"training": {"epochs": 1}}) is None and G.GazeAugmentation.from_config({}) is None
    assert G.GazeAugmentation.from_config({"training": {"image_augmentation": {"contrast": 0.1}}}) == G.GazeAugmentation(0.5, 0.2, 0.1)
    with pytest.raises(ValueError, match=r"unknown keys \['rotation'\]"):
        G.GazeAugmentation.from_config({"training": {"image_augmentation": {"rotation": 10}}})
    with pytest.raises(ValueError, match="must be a mapping"):
        G.GazeAugmentation.from_config({"training": {"image_augmentation": 0.5}})
    with pytest.raises(ValueError, match="brightness must lie"):
        G.GazeAugmentation.from_config({"training": {"image_augmentation": {"brightness": 1.5}}})


FAKE = 0x1000       # never dereferenced: every call below is refused before a launch


def resize_args(**over):
    a = dict(data=FAKE, off=FAKE, h=FAKE, w=FAKE, mid_off=FAKE, tabs=FAKE, htab=FAKE, vtab=FAKE, sum_h=40, n=2, max_h=30, F=16, W=24,
             ws=FAKE, ws_bytes=1 << 20, store=FAKE)
    a.update(over)
    desc = L.GazeResizeDesc(a["data"], a["off"], a["h"], a["w"], a["mid_off"], a["tabs"], a["htab"], a["vtab"], a["sum_h"], a["n"],
                            a["max_h"], a["F"], a["W"])
    return ctypes.byref(desc), a["ws"], a["ws_bytes"], a["store"], 0


def test_resize_refusals_run_without_a_gpu():
    cases = [(dict(data=0), "null pointer"), (dict(vtab=0), "null pointer"), (dict(ws=0), "null pointer"), (dict(store=0), "null pointer"),
             (dict(n=0), "n_images=0"), (dict(F=7), r"F=7 outside \[8, 512\]"), (dict(W=513), r"W=513 outside \[8, 512\]"),
             (dict(max_h=4097), r"max_h=4097 outside \[1, 4096\]"), (dict(sum_h=1), "sum_h=1 is not the sum of 2 heights"),
             (dict(sum_h=2 * 4096 + 1), "sum_h=8193"), (dict(ws_bytes=3 * 24 * 40 + 31), "need 2912 workspace bytes, the workspace has 2911"),
             (dict(data=FAKE + 4), "16-byte boundaries"), (dict(store=FAKE + 8), "16-byte boundaries")]
    for over, match in cases:
        with pytest.raises(L.EgError, match="eg_gaze_resize: .*" + match):
            L.call("eg_gaze_resize", *resize_args(**over))
    assert L.gaze_resize_workspace_bytes(2, 40, 24) == 3 * 24 * 40 + 32
    for bad in ((0, 40, 24), (2, 1, 24), (2, 2 * 4096 + 1, 24), (2, 40, 7), (2, 40, 513)):
        assert L.gaze_resize_workspace_bytes(*bad) == -1


def batch_args(**over):
    a = dict(store=FAKE, n_images=4, F=16, W=24, pair_img=FAKE, win_pair=FAKE, order=FAKE, order_len=11, first=3, n=5, norm=FAKE, lo=1, hi=2,
             hflip=0.5, brightness=0.2, contrast=0.2, factors=0, img1=FAKE, img2=FAKE, rgb1=0, rgb2=0)
    a.update(over)
    return tuple(a.values()) + (0,)


def test_batch_refusals_run_without_a_gpu():
    cases = [(dict(store=0), "null pointer"), (dict(pair_img=0), "null pointer"), (dict(win_pair=0), "null pointer"), (dict(order=0), "null pointer"),
             (dict(norm=0), "null pointer"), (dict(img1=0), "null pointer"), (dict(img2=0), "null pointer"), (dict(n=0), "n=0"),
             (dict(n_images=0), "n_images=0"), (dict(F=520), "F=520 outside"), (dict(W=4), "W=4 outside"),
             (dict(first=-1), r"samples \[-1, -1 \+ 5\) outside the order of 11"), (dict(first=7), r"samples \[7, 7 \+ 5\) outside the order of 11"),
             (dict(hflip=1.5), r"hflip_p=1.5 outside \[0, 1\]"), (dict(hflip=-0.5), "hflip_p=-0.5"), (dict(hflip=float("nan")), "hflip_p=nan"),
             (dict(brightness=1.0), r"brightness=1 outside \[0, 1\)"), (dict(brightness=float("nan")), "brightness=nan"),
             (dict(contrast=-0.1), "contrast=-0.1 outside"), (dict(contrast=float("inf")), "contrast=inf"),
             (dict(rgb1=FAKE), "rgb1 and rgb2 come together")]
    for over, match in cases:
        with pytest.raises(L.EgError, match="eg_gaze_batch: .*" + match):
            L.call("eg_gaze_batch", *batch_args(**over))


def test_store_refuses_what_the_kernels_do_not_serve():
    ok = np.zeros((5, 6, 3), np.uint8)
    for images, size, match in (([np.zeros((1, 4097, 3), np.uint8)], 16, "1x4097, served are sides of 1 to 4096"),
                                ([ok, np.zeros((4097, 2, 3), np.uint8)], 16, "image 1 is 4097x2"),
                                ([np.zeros((0, 5, 3), np.uint8)], 16, "0x5"), ([np.zeros((5, 6), np.uint8)], 16, r"uint8 \(h, w, 3\)"),
                                ([np.zeros((5, 6, 4), np.uint8)], 16, r"uint8 \(h, w, 3\)"), ([ok.astype(np.float32)], 16, "float32"),
                                ([ok], 7, "size 7x7"), ([ok], (16, 513), "size 16x513")):
        with pytest.raises(ValueError, match=match):
            G.GazeImageStore.from_arrays(images, size, device="cpu")
    with pytest.raises(ValueError, match=r"uint8 \[N, F, W, 3\]"):
        G.GazeImageStore(torch.zeros(2, 16, 24, 3))
    with pytest.raises(ValueError, match=r"integer \[3, 2\]"):
        G.validate_pair_img(np.zeros((2, 2), np.int64), 3, 4)
    with pytest.raises(ValueError, match=r"pair 1 names images \[0, 4\] of a store of 4"):
        G.validate_pair_img([[0, 1], [0, 4], [2, 3]], 3, 4)
    assert G.validate_pair_img([[0, 1], [3, 3]], 2, 4).dtype == np.int32


# ---------------------------------------------------------------------------------------------------------------
# the trainer's file side
# ---------------------------------------------------------------------------------------------------------------
def test_pair_filtering_and_image_numbering(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from eyegaze_multimodal_amd import train_multimodal_fuzzy_fusion as M
    from eyegaze_multimodal_amd.data import build_recording_store
    rng = np.random.default_rng(3)
    img_dir, eeg_dir = tmp_path / "img", tmp_path / "eeg"
    img_dir.mkdir(), eeg_dir.mkdir()
    names = [f"P{i}" for i in range(6)]
    pixels = {}
    for n in names:
        np.savetxt(eeg_dir / f"{n}.csv", rng.normal(size=(4, 160)).astype(np.float32), delimiter=",")
        pixels[n] = rng.integers(0, 256, (9 + len(pixels), 13, 3), dtype=np.uint8)
        Image.fromarray(pixels[n]).save(img_dir / f"{n}.png")
    (img_dir / "P4.png").unlink()                                          # P4 has no image
    (eeg_dir / "P5.csv").unlink()                                          # P5 has no recording
    items = [dict(player1="P0", player2="P1", **{"class": "Single"}), dict(player1="P2", player2="P4", **{"class": "Single"}),
             dict(player1="P1", player2="P2", **{"class": "Cooperation"}), dict(player1="P5", player2="P0", **{"class": "Single"}),
             dict(player1="P3", player2="P3", **{"class": "Competition"}), dict(player1="P9", player2="P0", **{"class": "Single"})]
    kept = M.multimodal_items(items, img_dir, eeg_dir, ".png")
    assert [(it["player1"], it["player2"]) for it in kept] == [("P0", "P1"), ("P1", "P2"), ("P3", "P3")]
    assert M.multimodal_items(items, img_dir, eeg_dir) == []               # the reference's .jpg: none here
    label2id = {"Single": 0, "Competition": 1, "Cooperation": 2}
    idx_a = build_recording_store(kept[:2], eeg_dir, label2id, tmp_path / "a", window_size=64, stride=32)
    idx_b = build_recording_store(kept[2:], eeg_dir, label2id, tmp_path / "b", window_size=64, stride=32)
    assert idx_a["count"] == 8 and idx_b["count"] == 4
    paths, (tab_a, tab_b) = M.image_tables([idx_a, idx_b], img_dir, ".png")
    assert [p.name for p in paths] == ["P0.png", "P1.png", "P2.png", "P3.png"]
    assert tab_a.dtype == np.int32 and tab_a.tolist() == [[0, 1], [1, 2]] and tab_b.tolist() == [[3, 3]]
    for p in paths:
        assert np.array_equal(G.load_rgb(p), pixels[p.stem])
    Image.fromarray(pixels["P0"][..., 0]).save(img_dir / "grey.png")
    assert np.array_equal(G.load_rgb(img_dir / "grey.png"), np.repeat(pixels["P0"][..., :1], 3, axis=2))      # convert('RGB')
    broken = dict(idx_b, pairs=idx_b["pairs"] + [{"offset": 0, "length": 64, "dataset_idx": 9}])
    with pytest.raises(ValueError, match="pair 1 has no window"):
        M.image_tables([broken], img_dir, ".png")
    for size in (12, 226, 520, 4):
        with pytest.raises(ValueError, match=f"data.image_size = {size}"):
            M.check_image_size(size)
    assert [M.check_image_size(s) for s in (8, 16, 224, 512)] == [8, 16, 224, 512]
