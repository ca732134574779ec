"""CPU tests (-m "not gpu") of gdrnet_amd.devargs, the argument checks the pose-geometry modules share: they need no GPU and no library."""
import numpy as np
import pytest
import torch

from gdrnet_amd import bop_metrics as BM, cabi, devargs, pose_metrics as PM


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def no_load(*a, **k):
        raise AssertionError("devargs must not load the library")

    monkeypatch.setattr(cabi, "load", no_load)


@pytest.mark.parametrize("bound, inclusive", [(4, False), (3, True)])   # both accept 0 .. 3
def test_index_vector_checks_length_and_range_on_the_host(bound, inclusive):
    ok = [3, 0, 2]
    dev, host = devargs.index_vector(ok, 3, bound, "cpu", "labels", inclusive=inclusive)
    assert host.dtype == np.int32 and host.flags["C_CONTIGUOUS"] and list(host) == ok
    assert dev.dtype == torch.int32 and dev.tolist() == ok
    with pytest.raises(ValueError):
        devargs.index_vector(ok, 4, bound, "cpu", "labels", inclusive=inclusive)       # wrong length
    with pytest.raises(ValueError):
        devargs.index_vector([0, -1, 2], 3, bound, "cpu", "labels", inclusive=inclusive)
    top = bound + 1 if inclusive else bound                                           # the first value outside
    with pytest.raises(ValueError):
        devargs.index_vector([0, top, 2], 3, bound, "cpu", "labels", inclusive=inclusive)
    assert list(devargs.index_vector([0, top - 1, 2], 3, bound, "cpu", "labels", inclusive=inclusive)[1]) == [0, top - 1, 2]
    assert list(devargs.index_vector([], 0, bound, "cpu", "labels", inclusive=inclusive)[1]) == []


def test_index_vector_takes_a_list_a_numpy_array_and_a_cpu_tensor_alike():
    want = np.array([2, 0, 1, 1], dtype=np.int32)
    for values in ([2, 0, 1, 1], np.array([2, 0, 1, 1], dtype=np.int64), torch.tensor([2, 0, 1, 1]), torch.tensor([[2, 0], [1, 1]], dtype=torch.int16)):
        dev, host = devargs.index_vector(values, 4, 3, "cpu", "labels")
        assert host.dtype == np.int32 and np.array_equal(host, want)
        assert dev.dtype == torch.int32 and np.array_equal(dev.numpy(), want)
    assert list(devargs.index_vector([7, 9], 2, None, "cpu", "labels")[1]) == [7, 9]   # no bound: the range is left to the library


def test_device_tensor_refuses_what_is_not_on_the_device():
    for t in (torch.zeros(2, 3, 3), np.zeros((2, 3, 3)), [[0.0] * 3] * 3, None):
        with pytest.raises(cabi.GdrnHipError, match="the renderer"):
            devargs.device_tensor(t, torch.float64, (-1, 3, 3), "R", "the renderer")
    with pytest.raises(cabi.GdrnHipError):
        devargs.poses(torch.zeros(2, 3, 3), torch.zeros(2, 3), torch.eye(3), "the renderer")


def test_per_row_K_broadcasts_one_matrix_and_checks_the_count():
    K = torch.arange(9.0, dtype=torch.float64).reshape(3, 3)
    out = devargs.per_row_K(K, 3)
    assert out.shape == (3, 3, 3) and out.is_contiguous() and all(torch.equal(out[i], K) for i in range(3))
    Kn = torch.arange(27.0, dtype=torch.float64).reshape(3, 3, 3)
    assert torch.equal(devargs.per_row_K(Kn, 3), Kn)
    assert devargs.per_row_K(K, 1).shape == (1, 3, 3)
    with pytest.raises(ValueError):
        devargs.per_row_K(Kn[:2], 3)
    with pytest.raises(ValueError):
        devargs.per_row_K(Kn, 2)


def test_both_model_tables_pack_their_points_alike():
    rng = np.random.default_rng(0)
    points, diameters = [rng.standard_normal((5, 3)), rng.standard_normal((7, 3))], [0.2, 0.3]
    a, b = PM.ModelTable(points, diameters, pad_value=7.0), BM.BopModelTable(points, diameters, pad_value=7.0)
    for t in (a, b):
        assert t.n_max == 7 and t.pts.shape == (2, 7, 3) and t.pts.dtype == np.float64 and t.npts.dtype == np.int32 and list(t.npts) == [5, 7]
        for c, p in enumerate(points):
            assert np.array_equal(t.pts[c, : len(p)], p) and np.all(t.pts[c, len(p):] == 7.0)
    assert a.n_max == b.n_max
    for k in ("pts", "npts", "diameter"):
        assert np.array_equal(getattr(a, k), getattr(b, k)) and getattr(a, k).dtype == getattr(b, k).dtype
    assert np.array_equal(a.diameter, diameters)
    # an empty class: the pose metrics accept it (a table row of padding), MSSD / MSPD have no value for it
    e = PM.ModelTable([points[0], np.zeros((0, 3))], diameters, pad_value=7.0)
    assert list(e.npts) == [5, 0] and e.n_max == 5 and np.all(e.pts[1] == 7.0)
    assert PM.ModelTable([np.zeros((0, 3))], [0.1]).n_max == 1
    with pytest.raises(ValueError):
        BM.BopModelTable([points[0], np.zeros((0, 3))], diameters)


def test_tables_name_what_they_upload():
    points = [np.zeros((2, 3))]
    assert PM.ModelTable.TABLES == ("pts", "npts", "diameter", "sym", "nsym", "is_sym")
    assert BM.BopModelTable.TABLES == ("pts", "npts", "diameter", "sym_R", "sym_t", "nsym")
    for t in (PM.ModelTable(points, [0.1]), BM.BopModelTable(points, [0.1])):
        tb = t.on("cpu")
        assert tuple(tb) == t.TABLES and t.on("cpu") is tb and all(np.array_equal(tb[k].numpy(), getattr(t, k)) for k in t.TABLES)
