"""CPU tests (-m "not gpu") of gdrnet_amd.pose_metrics: no CPU fallback, table packing, the workspace query and the formatting of the recall
table (the evaluator's big_tab, core/gdrn_modeling/gdrn_custom_evaluator.py:613-647) on hand-filled counters."""
import numpy as np
import pytest
import torch

from gdrnet_amd import cabi, pose_metrics as PM, synth


def _table(case="A", **kw):
    inp = synth.make_pose_metric_inputs(case)
    return inp, PM.ModelTable(inp["points"], inp["diameters"], inp["sym_infos"], inp["sym_classes"], **kw)


def test_pose_metrics_have_no_cpu_fallback():
    inp, table = _table()
    poses = [torch.from_numpy(inp[k]) for k in ("R_est", "t_est", "R_gt", "t_gt", "K")]
    with pytest.raises(cabi.GdrnHipError):
        PM.pose_errors(table, *poses, inp["labels"])
    with pytest.raises(cabi.GdrnHipError):
        PM.PoseRecall(table, inp["obj_names"]).update(*poses, inp["labels"])
    with pytest.raises(cabi.GdrnHipError):
        PM.pose_errors(table, *[p.numpy() for p in poses], inp["labels"])


def test_model_table_packing():
    inp, t = _table(pad_value=7.0)
    assert t.num_classes == 3 and t.n_max == 1031 and t.k_max == 2
    assert t.pts.shape == (3, 1031, 3) and t.pts.dtype == np.float64 and t.npts.dtype == np.int32 and list(t.npts) == [1031, 257, 1]
    for c, p in enumerate(inp["points"]):
        assert np.array_equal(t.pts[c, : len(p)], p) and np.all(t.pts[c, len(p):] == 7.0)
    assert t.sym.shape == (3, 2, 3, 3) and list(t.nsym) == [0, 2, 1] and list(t.is_sym) == [0, 1, 1]
    assert inp["sym_infos"][2].shape == (3, 3) and np.array_equal(t.sym[2, 0], inp["sym_infos"][2]) and not t.sym[2, 1].any()   # bare 3x3 -> [1,3,3]
    assert np.array_equal(t.sym[1], inp["sym_infos"][1]) and not t.sym[0].any()
    assert np.array_equal(t.diameter, [0.2, 0.3, 0.1])
    t32 = PM.ModelTable([p.astype(np.float32) for p in inp["points"]], inp["diameters"])   # no symmetry information at all
    assert t32.pts.dtype == np.float64 and not t32.is_sym.any() and t32.sym.shape == (3, 1, 3, 3) and not t32.nsym.any()
    with pytest.raises(ValueError):
        PM.ModelTable(inp["points"], inp["diameters"][:2])
    with pytest.raises(ValueError):
        PM.ModelTable(inp["points"], inp["diameters"], sym_classes=(3,))
    with pytest.raises(ValueError):
        PM.PoseRecall(t, ["a", "b"])


def test_synthetic_pose_metric_inputs_are_deterministic_and_cover_the_edge_rows():
    a, b = synth.make_pose_metric_inputs("A"), synth.make_pose_metric_inputs("A")
    for k in ("R_est", "t_est", "R_gt", "t_gt", "K", "labels"):
        assert np.array_equal(a[k], b[k]) and a[k].dtype in (np.float64, np.int64)
    assert len(a["labels"]) == 67 and sum(a["missing"].values()) == 8
    assert np.allclose(a["R_est"] @ a["R_est"].transpose(0, 2, 1), np.eye(3), atol=1e-12)
    assert np.array_equal(a["R_est"][[0, 4]], a["R_gt"][[0, 4]]) and np.array_equal(a["t_est"][[0, 4]], a["t_gt"][[0, 4]])
    assert np.array_equal(a["R_est"][7], a["R_gt"][7] @ a["sym_infos"][1][0]) and np.array_equal(a["R_est"][10], a["R_gt"][10] @ a["sym_infos"][1][1])
    bb = synth.make_pose_metric_inputs("B")
    assert len(bb["labels"]) == 3 and bb["points"][0].shape == (8195, 3) and bb["sym_classes"] == (0,)


def test_workspace_query_is_positive_and_monotone():
    lib = cabi.load()
    ws = lib.gdrn_pose_metrics_workspace_bytes
    assert ws(1, 1) > 0 and ws(64, 16384) > 0
    assert ws(0, 100) == -1 and ws(4, 0) == -1 and ws(-1, -1) == -1
    sizes = (1, 2, 1023, 1024, 1025, 8195, 16384, 1 << 20)
    for n in (1, 3, 64, 4096):
        vals = [ws(n, m) for m in sizes]
        assert all(x <= y for x, y in zip(vals, vals[1:])) and vals[0] < vals[-1]
        assert all(ws(n, m) < ws(n + 1, m) for m in sizes)
    assert ws(1 << 20, 1 << 20) > 2 ** 31   # a long long, not an int


def test_summary_formatting_on_hand_filled_counters():
    names = ["pear", "apple", "fig", "never_seen"]
    hits = np.zeros((4, 15), dtype=np.int64)
    hits[0] = np.arange(15) % 4          # pear: 3 predictions + 1 missing
    hits[1] = 3                          # apple: all three hit everything
    seen = np.array([4, 3, 5, 0])
    err_cnt = np.array([3, 3, 0, 0])     # fig: five ground-truth instances, not one prediction
    re_sum, te_sum = np.array([3.0, 37.02, 0.0, 0.0]), np.array([0.06, 0.3, 0.0, 0.0])
    rows = PM.format_table(names, hits, seen, re_sum, te_sum, err_cnt)
    assert rows[0] == ["objects", "apple", "fig", "pear", "Avg(3)"]
    assert [r[0] for r in rows[1:]] == list(PM.METRIC_NAMES) + ["re", "te"] and len(rows) == 18
    assert rows[1] == ["ad_2", "100.00", "0.00", "0.00", "33.33"]
    assert rows[2] == ["ad_5", "100.00", "0.00", "25.00", "41.67"]
    assert rows[4] == ["rete_2", "100.00", "0.00", "75.00", "58.33"]
    assert rows[16] == ["re", "12.34", "nan", "1.00", "nan"]
    assert rows[17] == ["te", "0.10", "nan", "0.02", "nan"]
    assert all(isinstance(c, str) for r in rows for c in r)
    # nothing seen at all: the header and empty rows, as the evaluator's loop over zero objects
    empty = PM.format_table(names, hits * 0, seen * 0, re_sum * 0, te_sum * 0, err_cnt * 0)
    assert empty[0] == ["objects", "Avg(0)"] and empty[1] == ["ad_2"] and empty[16] == ["re"]
    # a PoseRecall that was never updated summarises to the same
    _, table = _table()
    assert PM.PoseRecall(table, ["a", "b", "c"]).summarize() == PM.format_table(["a", "b", "c"], np.zeros((3, 15)), np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3))
