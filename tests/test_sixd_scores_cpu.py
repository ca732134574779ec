"""CPU tests (-m "not gpu") of gdrnet_amd.sixd_scores: the host oracle (tests/sixd_host.py) against golden G18 (the reference's add / adi / re_sym /
te_sym / arp_2d_sym, match_poses and calc_recall on the fixture of synth.make_sixd_score_inputs), the table strings from hand-made counters,
select_top_estimates, the checks that raise before any launch, and the exported symbols."""
import os

import numpy as np
import pytest
import torch

import sixd_host as SH
from gdrnet_amd import bop_metrics as BM
from gdrnet_amd import cabi, sixd_scores as SS, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gdrn_ad_errors_workspace_bytes", "gdrn_ad_errors", "gdrn_sym_errors_workspace_bytes", "gdrn_sym_errors",
               "gdrn_score_recall_accumulate")


@pytest.fixture(scope="module")
def g18(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g18_sixd_scores.npz")))


@pytest.fixture(scope="module")
def inp():
    return synth.make_sixd_score_inputs()


@pytest.fixture(scope="module")
def host(inp):
    return SH.errors_all(inp)


def test_host_errors_equal_the_reference(g18, inp, host):
    assert int(g18["sym/seed"]) == synth.SIXD_SCORE_SEEDS["sym"]
    SH.check_errors(*host, g18["sym/err"], "host restatement")
    ad, sym = host
    assert not ad[6].any() and sym[6, 0] <= 1e-5 and not sym[6, 1:].any()   # est = gt, the single point, identity only (re: arccos next to 1)
    assert ad[0, 0] == 0.0 and ad[0, 1] == 0.0 and abs(sym[0, 0] - 360.0 / 315) < 1e-9   # est = gt, continuous symmetry: no identity in the set, one step
    for i in (5, 8):   # est = gt o S_k: zero against the set, far from it against the plain pose (te_sym as the reference runs it is no distance: not 0)
        assert sym[i, 0] <= 1e-5 and sym[i, 2] <= 1e-10 and ad[i, 0] > 0.01 and sym[i, 1] > 1e-3
    # te_sym is the reference's broadcast value: sqrt(3) |t_gt - t_est| on the class with the identity only
    rows2 = inp["labels"] == 2
    plain = np.sqrt(((inp["t_gt"] - inp["t_est"]) ** 2).sum(1))
    assert np.all(np.abs(sym[rows2, 1] - np.sqrt(3.0) * plain[rows2]) <= 1e-13) and np.all(np.abs(g18["sym/err"][rows2, 3] / 1000 - np.sqrt(3.0) * plain[rows2]) <= 1e-13)


def test_host_decisions_and_recalls_equal_the_reference(g18, inp, host):
    fl = SH.flags(*host, inp["labels"], inp["diameters"], inp["sym_classes"])
    assert fl.shape == g18["sym/match"].shape == (41, 51) and np.array_equal(fl, g18["sym/match"])
    assert [c.split(":")[0] for c in g18["sym/columns"]] == [name for name, ths in SH.TYPES for _ in ths]
    cnt = SH.recall_counts(*host, inp["labels"], inp["diameters"], inp["sym_classes"], 4, inp["missing"])
    assert np.array_equal(cnt["seen"], g18["sym/targets"]) and list(cnt["seen"]) == [13, 10, 11, 10]
    assert np.array_equal(cnt["hits"] / cnt["seen"][:, None].astype(np.float64), g18["sym/recall"])
    # the fixture takes both branches of "ad", and they differ: class 3 (add) and class 0 (adi) have rows only one of the two accepts
    sym_rows = np.isin(inp["labels"], inp["sym_classes"])
    assert sym_rows.any() and (~sym_rows).any() and set(inp["sym_classes"]) == {0, 1}
    assert np.array_equal(fl[sym_rows, 20:30], fl[sym_rows, 10:20]) and np.array_equal(fl[~sym_rows, 20:30], fl[~sym_rows, 0:10])
    assert (fl[:, 0:10] != fl[:, 10:20])[inp["labels"] == 3].any() and (fl[:, 0:10] != fl[:, 10:20])[inp["labels"] == 0].any()
    for k in range(51):   # every column decides something
        assert fl[:, k].any() and (k == 41 or not fl[:, k].all())
    assert SS.score_tables(inp["obj_names"], **cnt) == SH.tables(inp["obj_names"], **cnt)


def test_tables_from_hand_made_counters():
    hits = np.zeros((4, 51), dtype=np.int64)
    seen = np.array([4, 0, 2, 3])            # "pear" 4 targets | "never" none | "plum" 2 | "lost": 3 targets, not one estimate
    hits[0, 0:10] = [0, 1, 1, 2, 2, 3, 3, 4, 4, 4]   # AUCadd
    hits[2, 0:10] = 2
    hits[0, 30], hits[2, 30] = 1, 2                  # ABSadd
    hits[0, 33:36], hits[2, 33:36] = [1, 2, 4], [0, 1, 1]   # add
    hits[0, 45:48] = [0, 3, 4]                       # reteS
    t = SS.score_tables(["pear", "never", "plum", "lost"], hits, seen)
    assert list(t) == [name for name, _, _ in SS.SCORE_TYPES] == [name for name, _ in SH.TYPES] and len(t) == 12
    assert t["AUCadd"] == [["objects", "AUCadd_10"], ["pear", "60.00"], ["plum", "100.00"], ["lost", "0.00"], ["Avg(3)", "53.33"]]
    assert t["ABSadd"] == [["objects", "ABSadd_2"], ["pear", "25.00"], ["plum", "100.00"], ["lost", "0.00"], ["Avg(3)", "41.67"]]
    assert t["add"] == [["objects", "add_0.020", "add_0.050", "add_0.100"], ["pear", "25.00", "50.00", "100.00"], ["plum", "0.00", "50.00", "50.00"],
                        ["lost", "0.00", "0.00", "0.00"], ["Avg(3)", "8.33", "33.33", "50.00"]]
    assert t["reteS"][0] == ["objects", "reteS_2", "reteS_5", "reteS_10"] and t["reteS"][1] == ["pear", "0.00", "75.00", "100.00"]
    assert t["projS"][0] == ["objects", "projS_2", "projS_5", "projS_10"] and t["teS"][0][1:] == ["teS_2", "teS_5", "teS_10"]
    assert t["AUCad"][0] == ["objects", "AUCad_10"] and t["ABSadi"][0] == ["objects", "ABSadi_2"] and t["adi"][0][1] == "adi_0.020"
    assert all(isinstance(c, str) for rows in t.values() for r in rows for c in r) and not any("never" in r for rows in t.values() for r in rows)
    assert t == SH.tables(["pear", "never", "plum", "lost"], hits, seen)
    # a single-object run: the AUC table keeps its object and ends in Avg(1); the other types, like the reference, have no average row
    one = SS.score_tables(["pear"], hits[:1], seen[:1])
    assert one["AUCadd"] == [["objects", "AUCadd_10"], ["pear", "60.00"], ["Avg(1)", "60.00"]]
    assert one["ABSadd"] == [["objects", "ABSadd_2"], ["pear", "25.00"]] and one["add"] == [["objects", "add_0.020", "add_0.050", "add_0.100"],
                                                                                             ["pear", "25.00", "50.00", "100.00"]]
    assert one == SH.tables(["pear"], hits[:1], seen[:1])
    none = SS.score_tables(["a", "b"], hits[:2] * 0, [0, 0])
    assert none["AUCadd"] == [["objects", "AUCadd_10"]] and none["reS"] == [["objects", "reS_2", "reS_5", "reS_10"]]


def test_select_top_estimates():
    keys = [(1, 5, 2), (1, 5, 2), (1, 5, 3), (1, 5, 2), (2, 0, 2), (1, 5, 3), (1, 5, 2)]
    scores = [0.3, 0.9, 0.5, 0.9, 0.1, 0.5, 0.95]
    assert SS.select_top_estimates(keys, scores).tolist() == [6, 2, 4]                      # the earlier one of the two 0.5s
    assert SS.select_top_estimates(keys, scores, 2).tolist() == [6, 1, 2, 5, 4]             # 0.9 twice: row 1 before row 3; one estimate where two may go
    assert SS.select_top_estimates(keys, scores, 3).tolist() == [6, 1, 3, 2, 5, 4]
    assert SS.select_top_estimates(keys, scores, {(1, 5, 2): 2, (2, 0, 2): 0}).tolist() == [6, 1, 2]
    assert SS.select_top_estimates(np.array(keys), np.array(scores)).tolist() == [6, 2, 4]  # rows of an integer array
    assert SS.select_top_estimates(["a", "b", "a"], [1.0, 1.0, 1.0]).tolist() == [0, 1]
    got = SS.select_top_estimates([], [])
    assert got.dtype == np.int64 and got.shape == (0,)
    for n in (1, 2, 3):
        assert SS.select_top_estimates(keys, scores, n).tolist() == SH.top_estimates(keys, scores, n)
    # a target without an estimate has no key here: nothing is selected for it, and the recall state counts it through add_missing
    assert (3, 1, 9) not in keys and len(SS.select_top_estimates(keys, scores)) == len(set(keys))
    with pytest.raises(ValueError):
        SS.select_top_estimates(keys, scores[:3])
    with pytest.raises(ValueError):
        SS.select_top_estimates(keys, scores, -1)


def test_no_cpu_fallback_and_checks_before_any_launch(inp):
    t = BM.BopModelTable(inp["points"], inp["diameters"], inp["syms"])
    poses = [torch.from_numpy(inp[k]) for k in ("R_est", "t_est", "R_gt", "t_gt", "K")]
    with pytest.raises(cabi.GdrnHipError):
        SS.ad_errors(t, *poses[:4], inp["labels"])
    with pytest.raises(cabi.GdrnHipError):
        SS.sym_errors(t, *poses, inp["labels"])
    rec = SS.ScoreRecall(t, inp["obj_names"], inp["sym_classes"], inp["im_width"])
    assert list(rec.ad_is_adi) == [1, 1, 0, 0] and rec.ad_is_adi.dtype == np.int32
    with pytest.raises(cabi.GdrnHipError):
        rec.update(torch.zeros(3, 2), torch.zeros(3, 3), [0, 1, 2])
    with pytest.raises(cabi.GdrnHipError):
        rec.add_missing(0, 1)
    with pytest.raises(ValueError):
        rec.add_missing(4, 1, device="cpu")
    for bad in (dict(obj_names=["a", "b"]), dict(sym_classes=[4]), dict(sym_classes=[-1]), dict(im_width=0)):
        kw = dict(obj_names=inp["obj_names"], sym_classes=inp["sym_classes"], im_width=640)
        kw.update(bad)
        with pytest.raises(ValueError):
            SS.ScoreRecall(t, kw["obj_names"], kw["sym_classes"], kw["im_width"])
    cnt = rec.counters()   # before any update: zeros, and tables without an object
    assert cnt["hits"].shape == (4, 51) and not cnt["hits"].any() and not cnt["seen"].any() and rec.summarize()["AUCad"] == [["objects", "AUCad_10"]]
    # the C entry points themselves: a label outside its range is refused on the host copy, before a stream or a device pointer is touched
    lib = cabi.load()
    one = np.ones(64, dtype=np.float64)
    p = one.ctypes.data
    for labels in ([0, 4], [-1, 0]):
        lab = np.array(labels, dtype=np.int32)
        assert lib.gdrn_ad_errors(p, p, p, p, p, lab.ctypes.data, 2, p, p, 8, 4, p, p, None) == -1
        assert lib.gdrn_sym_errors(p, p, p, p, p, p, lab.ctypes.data, 2, p, p, 8, p, p, p, 3, 4, p, p, None) == -1
        assert lib.gdrn_score_recall_accumulate(p, p, p, lab.ctypes.data, 2, p, p, 4, p, p, None) == -1
    lab = np.zeros(2, dtype=np.int32)
    assert lib.gdrn_ad_errors(p, p, p, p, p, lab.ctypes.data, 0, p, p, 8, 4, p, p, None) == -1
    assert lib.gdrn_ad_errors(p, p, p, p, p, lab.ctypes.data, 2, p, p, 0, 4, p, p, None) == -1
    assert lib.gdrn_ad_errors(None, p, p, p, p, lab.ctypes.data, 2, p, p, 8, 4, p, p, None) == -1
    assert lib.gdrn_ad_errors(p, p, p, p, p, None, 2, p, p, 8, 4, p, p, None) == -1
    assert lib.gdrn_sym_errors(p, p, p, p, p, p, lab.ctypes.data, 2, p, p, 8, p, p, p, 0, 4, p, p, None) == -1
    assert lib.gdrn_sym_errors(p, p, p, p, None, p, lab.ctypes.data, 2, p, p, 8, p, p, p, 3, 4, p, p, None) == -1
    assert lib.gdrn_score_recall_accumulate(p, p, p, lab.ctypes.data, 2, p, None, 4, p, p, None) == -1
    assert lib.gdrn_score_recall_accumulate(p, p, p, lab.ctypes.data, 0, p, p, 4, p, p, None) == -1
    big = np.zeros(65536, dtype=np.int32)   # more rows than a launch indexes: refused as a shape, after the label check
    assert lib.gdrn_ad_errors(p, p, p, p, p, big.ctypes.data, 65536, p, p, 8, 4, p, p, None) == -2
    assert lib.gdrn_sym_errors(p, p, p, p, p, p, big.ctypes.data, 65536, p, p, 8, p, p, p, 3, 4, p, p, None) == -2


def test_workspace_queries():
    lib = cabi.load()
    a, s = lib.gdrn_ad_errors_workspace_bytes, lib.gdrn_sym_errors_workspace_bytes
    assert a(1, 1) == 16 and a(41, 8195) == 41 * 2 * 9 * 8 and a(3, 1024) == 3 * 2 * 8 and a(3, 1025) == 3 * 4 * 8
    assert a(0, 1) == -1 and a(1, 0) == -1
    assert s(1, 1, 1) == (2 + 3) * 8 and s(41, 8195, 314) == 41 * (2 * 8195 + 3 * 40) * 8 and s(2, 5, 8) == 2 * (10 + 3) * 8 and s(2, 5, 9) == 2 * (10 + 6) * 8
    assert s(0, 1, 1) == -1 and s(1, 0, 1) == -1 and s(1, 1, 0) == -1
    assert s(65535, 1 << 20, 314) > 2 ** 31   # a long long, not an int


def test_new_symbols_are_exported_by_both_builds_and_declared():
    header = open(os.path.join(ROOT, "include", "gdrn_hip.h")).read()
    for lib in (cabi.load(), cabi.load(cabi.F16)):
        for name in NEW_SYMBOLS:
            assert name in cabi.EXPORTS and name in cabi._SIGS and hasattr(lib, name) and f" {name}(" in header
    for name in NEW_SYMBOLS:
        assert (name in cabi._RET_LL) == name.endswith("_bytes")
    assert f"GDRN_SIXD_AD_SLAB {SS.AD_SLAB}" in header and f"GDRN_SIXD_AD_TILE {SS.AD_TILE}" in header
    assert f"GDRN_SIXD_SYM_SLAB {SS.SYM_SLAB}" in header and f"GDRN_SIXD_NFLAGS {SS.NFLAGS}" in header and "GDRN_ABI_VERSION 5" in header
    assert SS.NFLAGS == SH.NFLAGS == 51 and sum(len(thr) for _, thr, _ in SS.SCORE_TYPES) == 51
    assert [col for _, _, col in SS.SCORE_TYPES] == list(np.cumsum([0] + [len(thr) for _, thr, _ in SS.SCORE_TYPES])[:-1])
    assert np.array_equal(SS.AUC_THS_CM, np.arange(1, 11)) and "sixd_scores.hip" in __import__("gdrnet_amd.build", fromlist=["SOURCES"]).SOURCES
    src = open(os.path.join(ROOT, "gdr-net_amd", "csrc", "sixd_scores.hip")).read()
    assert "__half" not in src and "bf16" not in src and "atomicAdd(&cnt" in src and "atomicAdd(hits" not in src   # nothing 16-bit; LDS counters only
