"""CPU tests of the device-resident data path's host side: the recording store against the shard builder and
the reference's enumeration (tests/golden/dataset_windows.npz), validate_store, the loaders' epoch order, the vote of
predict_recording and eg_window_gather's host checks.  No GPU, no compute through the C ABI."""
import copy
import ctypes
import json
from types import SimpleNamespace

import numpy as np
import pytest

from eyegaze_multimodal_amd import _lib as L
from eyegaze_multimodal_amd.data import (ResidentWindows, WindowShards, build_recording_store, build_window_shards, store_tables,
                                         validate_store)
from tests.test_data_host import FILES, ITEMS, LABEL2ID, STRIDE, W, Z, write_csvs


def fixture_store(tmp_path, from_csv=False):
    if from_csv:
        write_csvs(tmp_path)
    out = tmp_path / "store"
    index = build_recording_store(ITEMS, tmp_path if from_csv else None, LABEL2ID, out, W, STRIDE, recordings=None if from_csv else FILES)
    return out, index


@pytest.mark.parametrize("from_csv", [True, False])
def test_store_index_and_layout(tmp_path, from_csv):
    out, index = fixture_store(tmp_path, from_csv)
    assert index["count"] == 10 and index["channels"] == 6
    assert index["window_size"] == W and index["stride"] == STRIDE and index["label2id"] == LABEL2ID
    assert json.loads((out / "index.json").read_text()) == index
    assert [w["dataset_idx"] for w in index["windows"]] == Z["zscore/dataset_idx"].tolist()
    assert [w["start"] for w in index["windows"]] == Z["zscore/starts"].tolist()
    np.testing.assert_array_equal(np.load(out / "labels.npy"), Z["zscore/labels"])
    # starts 0..240 and 0..144 at stride 48 under window 128: (nwin - 1) * stride + W samples per pair, each sample once
    assert [p["length"] for p in index["pairs"]] == [368, 272]
    assert [p["offset"] for p in index["pairs"]] == [0, 2 * 6 * 368]
    assert [p["dataset_idx"] for p in index["pairs"]] == [0, 1]
    assert index["window_pair"] == [0] * 6 + [1] * 4
    store = np.load(out / "store.npy")
    assert store.shape == (7680,) and store.dtype == np.float32
    validate_store(index, store.shape[0])


def test_store_windows_are_the_shard_windows_bit_for_bit(tmp_path):
    out, index = fixture_store(tmp_path)
    sh = build_window_shards(ITEMS, None, LABEL2ID, tmp_path / "shards", W, STRIDE, shard_windows=4, recordings=FILES)
    raw = np.concatenate([np.load(tmp_path / "shards" / s["file"]) for s in sh["shards"]])
    assert {k: v for k, v in sh.items() if k != "shards"} == {k: v for k, v in index.items() if k not in ("pairs", "window_pair")}
    store = np.load(out / "store.npy")
    off, ln, wp, ws = store_tables(index)
    C = index["channels"]
    for j in range(index["count"]):
        p = wp[j]
        for who in range(2):
            for c in range(C):
                a = off[p] + (who * C + c) * ln[p] + ws[j]           # the address eg_window_gather states
                assert store[a:a + W].tobytes() == raw[j, who, c].tobytes()


def test_store_rejects_mixed_channel_counts(tmp_path):
    recs = {"a": np.zeros((4, 200), np.float32), "b": np.zeros((4, 200), np.float32), "c": np.zeros((5, 200), np.float32)}
    items = [{"player1": "a", "player2": "b", "class": "Single"}, {"player1": "c", "player2": "c", "class": "Single"}]
    with pytest.raises(ValueError):
        build_recording_store(items, None, LABEL2ID, tmp_path, W, STRIDE, recordings=recs)


def test_validate_store_rejects_what_the_kernel_would_trust(tmp_path):
    _, index = fixture_store(tmp_path)
    validate_store(index, 7680)
    bad = copy.deepcopy(index)
    bad["windows"][5]["start"] = 368 - W + 1                         # one sample past its pair's end
    with pytest.raises(ValueError, match="window 5"):
        validate_store(bad, 7680)
    bad = copy.deepcopy(index)
    bad["windows"][0]["start"] = -1
    with pytest.raises(ValueError, match="window 0"):
        validate_store(bad, 7680)
    with pytest.raises(ValueError, match="pair 1"):                  # the last pair ends past the store's end
        validate_store(index, 7679)
    bad = copy.deepcopy(index)
    bad["pairs"][1]["offset"] -= 1                                   # overlaps pair 0's last float
    with pytest.raises(ValueError, match="overlaps"):
        validate_store(bad, 7680)
    bad = copy.deepcopy(index)
    bad["window_pair"][9] = 2
    with pytest.raises(ValueError, match="names a pair"):
        validate_store(bad, 7680)


def test_resident_order_is_the_shard_loaders_order():
    for shuffle in (False, True):
        for seed, epoch in ((0, 0), (5, 1), (42, 3)):
            for rank, world in ((0, 1), (0, 2), (1, 2), (2, 3)):
                me = SimpleNamespace(n=10, shuffle=shuffle, seed=seed, epoch=epoch, rank=rank, world=world, B=3, drop_last=False)
                a, b = ResidentWindows._order(me), WindowShards._order(me)
                np.testing.assert_array_equal(a, b)
                ref = np.random.default_rng(seed + epoch).permutation(10) if shuffle else np.arange(10)
                np.testing.assert_array_equal(a, ref[rank::world])
                assert ResidentWindows.__len__(me) == WindowShards.__len__(me) == -(-len(a) // 3)
                me.drop_last = True
                assert ResidentWindows.__len__(me) == WindowShards.__len__(me) == (10 // world) // 3


def test_majority_vote_and_starts():
    from eyegaze_multimodal_amd.predict import majority_vote, recording_starts
    assert majority_vote([2, 2, 1, 0, 2], 3) == 2
    assert majority_vote([2, 1, 1, 2, 0], 3) == 1                    # tie between 1 and 2 -> the lowest id
    assert majority_vote([2, 0], 3) == 0
    assert majority_vote([1], 3) == 1
    assert recording_starts(1024 + 3 * 512, 1024, 512).tolist() == [0, 512, 1024, 1536]
    assert recording_starts(1024 + 3 * 512, 1024, 100).tolist() == list(range(0, 1537, 100))   # the 36-sample tail is dropped
    assert recording_starts(1023, 1024, 1).tolist() == []


def gather_args(**over):
    fake = 0x1000                                                    # never dereferenced: every case is refused before a launch
    d = dict(data=fake, pair_off=fake, pair_len=fake, win_pair=fake, win_start=fake, win_label=fake, n_pairs=2, n_windows=10,
             C=6, T=128, order=fake, order_len=10, first=0, n=4, eeg1=fake, eeg2=fake, labels=fake, mode=0)
    d.update(over)
    desc = L.WindowGatherDesc(d["data"], d["pair_off"], d["pair_len"], d["win_pair"], d["win_start"], d["win_label"], d["n_pairs"],
                              d["n_windows"], d["C"], d["T"])
    return (ctypes.byref(desc), d["order"], d["order_len"], d["first"], d["n"], d["eeg1"], d["eeg2"], d["labels"], d["mode"], 0)


@pytest.mark.parametrize("over,match", [
    (dict(data=0), "null pointer"), (dict(pair_off=0), "null pointer"), (dict(pair_len=0), "null pointer"),
    (dict(win_pair=0), "null pointer"), (dict(win_start=0), "null pointer"), (dict(order=0), "null pointer"),
    (dict(eeg1=0), "null pointer"), (dict(eeg2=0), "null pointer"),
    (dict(n=0), "bad shape"), (dict(C=0), "bad shape"), (dict(T=-1), "bad shape"),
    (dict(mode=2), "mode 2"), (dict(mode=-1), "mode -1"),
    (dict(T=16385), "16384"),
    (dict(first=-1), "outside the order"), (dict(first=7), "outside the order"), (dict(n=11), "outside the order"),
    (dict(win_label=0), "no win_label"),
])
def test_window_gather_host_checks(over, match):
    with pytest.raises(L.EgError, match=match):
        L.call("eg_window_gather", *gather_args(**over))


def test_window_gather_descriptor_mirrors_the_header():
    import re
    from tests.test_capi_symbols import REPO
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "eyegaze_hip.h").read_text(), flags=re.S)
    body = re.search(r"typedef struct eg_window_gather_desc \{(.*?)\} eg_window_gather_desc;", text, flags=re.S).group(1)
    names = [w for w in re.findall(r"\w+", body) if w not in ("const", "float", "int64_t", "int32_t")]   # declaration order
    assert names == [f[0] for f in L.WindowGatherDesc._fields_]
    assert ctypes.sizeof(L.WindowGatherDesc) == 6 * 8 + 4 * 4
    m = re.search(r"int\s+eg_window_gather\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m and len(m.group(1).split(",")) == len(L.SIGNATURES["eg_window_gather"]) == 10
