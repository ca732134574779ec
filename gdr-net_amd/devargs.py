"""Arguments of a device call, checked and brought into the form the C-ABI reads: what the pose-geometry modules (``pose_metrics``, ``pnp``,
``render``, ``bop_metrics``) do between their Python signature and the library.

One contract for all of them: a pose, an intrinsics matrix or a map must already be a device tensor (``cabi.GdrnHipError`` otherwise: there is no
CPU fallback); an index vector (labels, frames, counts) may come from the host or the device and is length- and range-checked ON THE HOST
(``ValueError``) before anything is loaded or launched.
"""
import numpy as np
import torch

from . import cabi


def no_fallback(what, where):
    """the error of an argument that is not on the device; ``where`` names the module in the sentence ("the renderer")"""
    return cabi.GdrnHipError(f"{where} runs on the GPU (no CPU fallback): {what} is not a device tensor")


def device_tensor(t, dtype, shape, what, where):
    """``t`` detached, as ``dtype``, reshaped to ``shape`` and contiguous (None keeps the dtype / the shape); fp32 -> fp64 widens exactly"""
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise no_fallback(what, where)
    t = t.detach()
    if dtype is not None:
        t = t.to(dtype)
    if shape is not None:
        t = t.reshape(shape)
    return t.contiguous()


def _host_indices(values, n, bound, what, inclusive):
    host = values.detach().cpu().numpy() if isinstance(values, torch.Tensor) else np.asarray(values)
    host = np.ascontiguousarray(host.reshape(-1).astype(np.int32))
    if n is not None and host.shape[0] != n:
        raise ValueError(f"{what}: {host.shape[0]} entries for {n} rows")
    if bound is not None and host.size and (host.min() < 0 or host.max() >= bound + bool(inclusive)):
        raise ValueError(f"{what} outside [0, {bound}{']' if inclusive else ')'}")
    return host


def index_vector(values, n, bound, device, what, inclusive=False):
    """(int32 device tensor, int32 host array) of ``n`` indices, each within [0, bound) -- [0, bound] with ``inclusive``, left to the library
    with ``bound`` None.  Values from the host (list / numpy / CPU tensor -- where a data loader has them) are uploaded to ``device``; a device
    tensor is copied back once for the check and otherwise used as it is."""
    host = _host_indices(values, n, bound, what, inclusive)
    if isinstance(values, torch.Tensor) and values.device.type == "cuda":
        return values.detach().reshape(-1).to(torch.int32).contiguous(), host
    return torch.from_numpy(host).to(device), host


def per_row_K(K, N, what="K"):
    """[N,3,3] contiguous from ``K`` [N,3,3], or one [3,3] for all rows"""
    K = K.reshape(-1, 3, 3)
    if K.shape[0] == 1 and N > 1:
        K = K.expand(N, 3, 3)
    if K.shape[0] != N:
        raise ValueError(f"{what}: {K.shape[0]} matrices for {N} rows (one per row, or one for all)")
    return K.contiguous()


def poses(R, t, K, where):
    """(R [N,3,3], t [N,3], K [N,3,3], N) as contiguous fp64 device tensors, N = the number of rotations"""
    R, t = device_tensor(R, torch.float64, (-1, 3, 3), "R", where), device_tensor(t, torch.float64, (-1, 3), "t", where)
    N = int(R.shape[0])
    K = per_row_K(device_tensor(K, torch.float64, (-1, 3, 3), "K", where), N)
    if t.shape[0] != N:
        raise ValueError("R and t need one entry per row")
    return R, t, K, N


def workspace(nbytes, device, what):
    """scratch of ``nbytes`` (the answer of a ``gdrn_*_workspace_bytes`` query, a negative one being its status), aligned for fp64"""
    nbytes = int(nbytes)
    if nbytes < 0:
        cabi.check(nbytes, what)
    return torch.empty(max((nbytes + 7) // 8, 1), dtype=torch.float64, device=device)


def stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def pack_points(points, diameters, pad_value, n_min=0):
    """(pts [C,n_max,3] fp64, npts [C] int32, n_max, diameter [C] fp64) from per-class [n_c,3] point clouds: n_max = the largest class (at
    least ``n_min``), ``pad_value`` in the rows beyond a class's own points"""
    clouds = [np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in points]
    npts = np.array([len(p) for p in clouds], dtype=np.int32)
    n_max = max(n_min, int(npts.max()))
    pts = np.full((len(clouds), n_max, 3), float(pad_value), dtype=np.float64)
    for c, p in enumerate(clouds):
        pts[c, : len(p)] = p
    return pts, npts, n_max, np.asarray(diameters, dtype=np.float64).reshape(len(clouds)).copy()


class DeviceTables:
    """Base of the per-class tables: numpy arrays as attributes, the ones named in ``TABLES`` uploaded once per device by ``on``."""

    TABLES = ()
    num_classes = 0

    def on(self, device):
        """the tables as device tensors (uploaded once per device)."""
        cache = self.__dict__.setdefault("_dev", {})
        key = str(device)
        if key not in cache:
            cache[key] = {k: torch.from_numpy(getattr(self, k)).to(device) for k in self.TABLES}
        return cache[key]

    def check_labels(self, labels):
        """labels (list / numpy / tensor) as a contiguous int32 host array, each within [0, num_classes): raises ValueError otherwise."""
        return _host_indices(labels, None, self.num_classes, "label", False)
