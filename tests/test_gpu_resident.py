"""GPU tests of the device-resident data path: eg_window_gather is eg_window_normalize's arithmetic behind another
addressing, so gathered windows are held BIT FOR BIT to eg_window_normalize on the same raw windows cut on the host; then the
loader against the reference's batches and against WindowShards, its rank partition and determinism, a training run with
data.resident against the shard run, and predict_recording against predict_windows."""
import ctypes
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

from eyegaze_multimodal_amd import _lib as L  # noqa: E402
from eyegaze_multimodal_amd._lib import call, ptr  # noqa: E402
from eyegaze_multimodal_amd.data import (DeviceRecordings, ResidentWindows, WindowShards, build_recording_store,  # noqa: E402
                                         build_window_shards)
from tests.test_data_host import FILES, ITEMS, LABEL2ID, STRIDE, W, Z  # noqa: E402

DEV = "cuda"
TOL = dict(atol=5e-6, rtol=0)      # the data path's tolerance against the reference's float32 reductions (test_gpu_data.py)


def beq(a: torch.Tensor, b: torch.Tensor) -> bool:
    """bit equality (torch.equal would call -0.0 and 0.0 equal)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def fixture_dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("resident")
    build_window_shards(ITEMS, None, LABEL2ID, root / "shards", W, STRIDE, shard_windows=4, recordings=FILES)
    build_recording_store(ITEMS, None, LABEL2ID, root / "store", W, STRIDE, recordings=FILES)
    return root / "shards", root / "store"


@pytest.mark.parametrize("mode,tag", [(0, "zscore"), (1, "car")])
def test_resident_loader_matches_reference_and_shard_batches(fixture_dirs, mode, tag):
    shards, store = fixture_dirs
    for B in (10, 4, 3):      # one batch; ragged tail; batches straddling the pair boundary
        ld = ResidentWindows(store, B, DEV, preprocessing=bool(mode))
        ref = list(WindowShards(shards, B, DEV, preprocessing=bool(mode)))
        got = list(ld)
        assert len(got) == len(ld) == len(ref)
        for g, r in zip(got, ref):
            assert beq(g["eeg1"], r["eeg1"]) and beq(g["eeg2"], r["eeg2"])
            assert g["labels"].dtype == torch.int64 and g["labels"].device.type == "cuda" and torch.equal(g["labels"], r["labels"])
            assert g["dataset_idx"] == r["dataset_idx"]
        np.testing.assert_allclose(torch.cat([g["eeg1"] for g in got]).cpu().numpy(), Z[f"{tag}/eeg1"], **TOL)
        np.testing.assert_allclose(torch.cat([g["eeg2"] for g in got]).cpu().numpy(), Z[f"{tag}/eeg2"], **TOL)
        np.testing.assert_array_equal(torch.cat([g["labels"] for g in got]).cpu().numpy(), Z[f"{tag}/labels"])
        assert sum((g["dataset_idx"] for g in got), []) == Z[f"{tag}/dataset_idx"].tolist()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("C,T,stride,N", [(8, 1024, 256, 64), (32, 1024, 256, 8), (5, 1000, 7, 3), (1, 64, 1, 5)])
def test_window_gather_is_window_normalize_bit_for_bit(C, T, stride, N, mode):
    """Two pairs of unequal length, the last window ending on the store's last float; (5, 1000, 7) and (1, 64, 1) put the row
    starts at every residue mod 4 floats.  The order is reversed, repeats a window and is entered at first = 2 with n < len."""
    g = torch.Generator().manual_seed(C)
    nwin = [N - N // 2, N // 2]
    if nwin[0] == nwin[1]:                                               # two pairs of unequal length
        nwin = [nwin[0] + 1, nwin[1] - 1]
    lens = [(n - 1) * stride + T for n in nwin]
    recs = [torch.randn(2, C, ln, generator=g) * 3e-5 + 1e-3 for ln in lens]   # test_window_normalize_full_size's data
    recs[0][0, :, :T] = 0.25                                             # window 0 of player 1 is constant: std = 0 -> exactly 0
    store = torch.cat([r.reshape(-1) for r in recs])
    pair_off = [0, recs[0].numel()]
    win_pair = [0] * nwin[0] + [1] * nwin[1]
    win_start = [i * stride for i in range(nwin[0])] + [i * stride for i in range(nwin[1])]
    assert pair_off[1] + (2 * C - 1) * lens[1] + win_start[-1] + T == store.numel()      # the last row ends the store
    if stride % 4:
        assert {(pair_off[p] + c * lens[p] + s) % 4 for p, s in zip(win_pair, win_start) for c in range(2 * C)} == {0, 1, 2, 3}
    win_label = np.arange(N) * 7 + 3
    raw = torch.stack([recs[p][:, :, s:s + T] for p, s in zip(win_pair, win_start)]).contiguous()     # [N, 2, C, T] cut on the host
    d = raw.to(DEV)
    r1, r2 = torch.empty(N, C, T, device=DEV), torch.empty(N, C, T, device=DEV)
    call("eg_window_normalize", ptr(d), ptr(r1), ptr(r2), N, C, T, mode, torch.cuda.current_stream().cuda_stream)
    order = [0, 1 % N] + list(range(N - 1, -1, -1)) + [N // 2, 0]
    first, n = 2, N + 1
    rec = DeviceRecordings(store.to(DEV), pair_off, lens, win_pair, win_start, win_label, C, T)
    order_dev = torch.tensor(order, dtype=torch.int32, device=DEV)
    e1, e2, lab = rec.gather(order_dev, first, n, mode)
    torch.cuda.synchronize()
    pick = torch.tensor(order[first:first + n], device=DEV)
    assert e1.shape == (n, C, T) and beq(e1, r1[pick]) and beq(e2, r2[pick])
    assert lab.cpu().tolist() == win_label[order[first:first + n]].tolist()
    assert torch.isfinite(e1).all() and torch.isfinite(e2).all()
    j0 = order[first:first + n].index(0)
    assert float(e1[j0].abs().max()) == 0.0
    # without labels: a descriptor that has no win_label
    rec2 = DeviceRecordings(rec.data, pair_off, lens, win_pair, win_start, None, C, T)
    f1, f2, none = rec2.gather(order_dev, first, n, mode)
    assert none is None and beq(f1, e1) and beq(f2, e2)


def test_resident_rank_partition_and_shuffle(fixture_dirs):
    seen = []
    for r in range(2):
        ld = ResidentWindows(fixture_dirs[1], 3, DEV, rank=r, world=2, shuffle=True, seed=5)
        ld.set_epoch(1)
        rows = torch.cat([b["eeg1"].cpu() for b in ld])
        assert rows.shape[0] == 5
        seen.append(rows)
    got = torch.cat(seen).numpy()
    ref = Z["zscore/eeg1"]
    used = set()      # every window appears exactly once across the two ranks (test_gpu_data.py's matching)
    for row in got:
        j = int(np.argmin(np.abs(ref - row[None]).reshape(len(ref), -1).max(1)))
        assert np.abs(ref[j] - row).max() < 1e-5 and j not in used
        used.add(j)
    assert len(used) == 10


def test_resident_walks_are_deterministic(fixture_dirs):
    ld = ResidentWindows(fixture_dirs[1], 4, DEV, shuffle=True, seed=3)
    walk = lambda: [torch.cat([b[k] for b in ld]) for k in ("eeg1", "eeg2", "labels")] + [sum((b["dataset_idx"] for b in ld), [])]
    a, b = walk(), walk()
    assert beq(a[0], b[0]) and beq(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3]
    o0 = ld._order()
    ld.set_epoch(1)
    o1 = ld._order()
    c = walk()
    assert not np.array_equal(o0, o1) and sorted(o0) == sorted(o1)
    inv0, inv1 = np.argsort(o0), np.argsort(o1)                          # back to window order: the same windows, bit for bit
    assert beq(a[0][inv0], c[0][inv1]) and beq(a[1][inv0], c[1][inv1]) and torch.equal(a[2][inv0], c[2][inv1])
    assert not beq(a[0], c[0])


def test_train_script_resident_equals_shards(tmp_path):
    """test_train_script_on_csv_recordings' set-up at 1 layer and 2 epochs, in-process, data.resident false and true: the same
    batches enter a deterministic step, so the per-epoch losses, the final metrics and the best model are equal bit for bit.
    Then predict.main on each run's test split, shard walk against the walk of the store: every array of the output file."""
    from eyegaze_multimodal_amd import predict as P
    from eyegaze_multimodal_amd import train_art as TA
    from tests.test_gpu_train import make_config
    rng = np.random.default_rng(0)
    eeg = tmp_path / "EEGseg"
    eeg.mkdir()
    names = ["Single", "Competition", "Cooperation"]
    items, tt = [], np.arange(1024 + 3 * 512) / 256.0
    for i in range(30):
        c = i % 3
        for who in (1, 2):
            x = 1e-5 * rng.standard_normal((8, len(tt))) + 2e-5 * np.sin(2 * np.pi * [6.0, 14.0, 31.0][c] * tt + rng.uniform(0, 6.28))
            np.savetxt(eeg / f"pair{i}_p{who}.csv", x.astype(np.float32), delimiter=",", fmt="%.7e")
        items.append({"player1": f"pair{i}_p1", "player2": f"pair{i}_p2", "class": names[c]})
    (tmp_path / "meta.json").write_text(json.dumps(items))
    runs = {}
    for resident in (False, True):
        out = tmp_path / f"resident_{resident}"
        out.mkdir()
        cfg = make_config(out, data={"synthetic": False, "metadata_path": str(tmp_path / "meta.json"), "eeg_base_path": str(eeg),
                                     "max_samples": None, "resident": resident},
                          model={"num_layers": 1}, training={"num_train_epochs": 2, "per_device_train_batch_size": 16,
                                                             "per_device_eval_batch_size": 16, "learning_rate": 5.0e-4})
        (out / "cfg.yaml").write_text(yaml.safe_dump(cfg))
        history = []
        final = TA.main(SimpleNamespace(config=str(out / "cfg.yaml"), dtype=None), history)
        ck = torch.load(out / "run" / "best_model.pt", weights_only=False)
        runs[resident] = (history, final, ck["model_state_dict"])
        # predict.main over the test split of the same run: the shard walk (through host memory) and the walk of the store
        P.main(SimpleNamespace(config=str(out / "cfg.yaml"), checkpoint=str(out / "run" / "best_model.pt"), out=str(out / "pred.npz"),
                               split="test", dtype=None, resident=resident, attention_stats="cross", attention_max_samples=200))
    pa, pb = np.load(tmp_path / "resident_False" / "pred.npz"), np.load(tmp_path / "resident_True" / "pred.npz")
    assert set(pa.files) == set(pb.files) and pa["logits"].shape == (24, 3) and "attn_mean_map" in pa.files
    for k in pa.files:
        assert pa[k].tobytes() == pb[k].tobytes(), k
    assert (tmp_path / "resident_False" / "run" / "window_shards" / "READY").exists()
    assert not (tmp_path / "resident_False" / "run" / "recording_store").exists()
    assert not (tmp_path / "resident_True" / "run" / "window_shards").exists()
    idx = json.loads((tmp_path / "resident_True" / "run" / "recording_store" / "train" / "index.json").read_text())
    assert idx["count"] == 24 * 4 and len(idx["pairs"]) == 24 and all(p["length"] == 1024 + 3 * 512 for p in idx["pairs"])
    (h0, f0, sd0), (h1, f1, sd1) = runs[False], runs[True]
    assert len(h0) == len(h1) == 2 and all(np.isfinite(v) for m in h0 for v in m.values())
    assert h0 == h1, (h0, h1)                                            # float == : every loss and metric of every epoch
    assert f0 == f1 and f0 is not None
    assert sd0.keys() == sd1.keys()
    assert all(torch.equal(sd0[k].view(torch.uint8), sd1[k].view(torch.uint8)) for k in sd0)


def test_predict_recording_equals_predict_windows():
    from eyegaze_multimodal_amd import DualEEGTransformer
    from eyegaze_multimodal_amd.predict import majority_vote, predict_recording, predict_windows
    from oracle import dual_eeg_oracle as O
    kw = dict(in_channels=8, num_classes=3, num_layers=1, max_len=256, use_spectrogram=False, use_ibs=False, use_cross_attention=True)
    model = DualEEGTransformer(**kw, compute_dtype="bf16")
    model.load_state_dict(O.synthetic_state_dict(O.ModelCfg(**kw), seed=7))
    model = model.to(DEV).eval()
    g = torch.Generator().manual_seed(11)
    Lr = 1024 + 3 * 512
    rec1, rec2 = torch.randn(8, Lr, generator=g) * 3e-5 + 1e-3, torch.randn(8, Lr, generator=g) * 3e-5 + 1e-3
    for stride, mode in ((512, 0), (100, 0), (100, 1)):
        starts = list(range(0, Lr - 1024 + 1, stride))
        raw = torch.stack([torch.stack([rec1[:, s:s + 1024], rec2[:, s:s + 1024]]) for s in starts]).to(DEV)
        n = len(starts)
        x1, x2 = torch.empty(n, 8, 1024, device=DEV), torch.empty(n, 8, 1024, device=DEV)
        call("eg_window_normalize", ptr(raw), ptr(x1), ptr(x2), n, 8, 1024, mode, torch.cuda.current_stream().cuda_stream)
        ref = predict_windows(model, x1, x2, None, batch_size=5)
        got = predict_recording(model, rec1.numpy() if stride == 512 else rec1, rec2, stride=stride, batch_size=5, preprocessing=bool(mode))
        assert got["starts"].tolist() == starts and set(got) == {"starts", "logits", "predictions", "vote"}
        assert beq(got["logits"], ref["logits"]) and torch.equal(got["predictions"], ref["predictions"])
        assert got["vote"] == majority_vote(ref["predictions"].cpu().numpy(), 3)
    whole = predict_recording(model, rec1, rec2)                         # stride = the window: two windows, the 512-sample tail dropped
    assert whole["starts"].tolist() == [0, 1024] and whole["logits"].shape == (2, 3)
    with pytest.raises(ValueError):
        predict_recording(model, rec1[:, :1000], rec2)
