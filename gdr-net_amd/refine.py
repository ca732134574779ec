"""Depth refinement of estimated poses on the device (csrc/icp.hip): projective point-to-plane ICP against observed depth frames.

The reference is RGB-only (``WITH_DEPTH=False``) and has no counterpart; this is the usual last step of an RGB-D entry between the network's
pose (or ``pnp.poses_from_maps``) and the metric modules.  Per iteration the model is rendered under the current pose (``render.render_depth``'s
launch), every pixel where the render and the observation lie within ``dist_gate`` of each other and the observation has a normal becomes a
pair, and the 6 x 6 point-to-plane normal equations of every estimate are summed and solved; the pose is updated by left multiplication.  The
association is by pixel: it refines estimates that already overlap the object within ``dist_gate`` -- an estimate further off along its viewing
ray (the usual error of an RGB-only pose) goes through ``depth_align`` first, or through ``refine_rgbd``, which runs both.  ``icp_refine``
itself has no silhouette term: flat-faced objects keep their sliding directions and come back with ok = 0; ``icp_refine_sil`` (below) adds
one from the observed instance mask.  There are no robust weights.  The arithmetic is stated with the entry
points in ``include/gdrn_hip.h``; all of it is fp64, sums have a fixed order (the same call gives the same bits; the instances of a batch do
not influence each other).  Nothing is read back inside ``icp_refine``.  There is no CPU fallback.

``depth_align`` (csrc/depth_align.hip) is that coarse step: the estimate is shifted along its viewing ray by the exact median of observed
minus rendered depth over the pixels where both exist and differ by at most ``gate``, a fixed number of times.  It corrects depth only: there
is no lateral alignment, no mask gate and no robust weighting beyond the median itself; the silhouette term lives in ``icp_refine_sil``.

``icp_refine_sil`` (csrc/silhouette.hip) is the ICP with a silhouette term: the contour of the observed instance mask -- the detector's or the
network's own mask head's -- is turned once per call into an exact distance transform with the index of the nearest contour pixel
(``contour_transform``); per iteration every contour pixel of the render within ``sil_gate`` pixels of the observed contour adds two
point-to-ray equations (``silhouette_equations``), and ``sil_weight`` times their system is added to the depth term's before the solve.  That
fixes the directions a plate or a cube seen on two faces leaves open.  Contour pixels that border a nearer observed surface (an occluder) are
no contour, and render pixels hidden behind a nearer observation are no pairs.  The reference has no counterpart.
"""
import torch

from . import cabi, devargs, render

WHERE = "the depth refinement"   # (this module in devargs' error sentence)
RUNNING, CONVERGED, DEGENERATE = 0, 1, 2   # GDRN_ICP_RUNNING, GDRN_ICP_CONVERGED, GDRN_ICP_DEGENERATE


def _scene(depth_scene):
    """the observed frames [F,H,W] fp32, on the device and contiguous"""
    if not isinstance(depth_scene, torch.Tensor) or depth_scene.device.type != "cuda":
        raise devargs.no_fallback("depth_scene", WHERE)
    if depth_scene.dtype != torch.float32:
        raise ValueError(f"depth_scene is {depth_scene.dtype}: torch.float32 (metres)")
    if depth_scene.dim() != 3 or min(depth_scene.shape[1:]) < 1:
        raise ValueError("depth_scene must be [F, H, W] with H and W of at least 1")
    return devargs.device_tensor(depth_scene, None, None, "depth_scene", WHERE)


def _gates(dist_gate, normal_gate):
    dist_gate, normal_gate = float(dist_gate), float(normal_gate)
    if not dist_gate > 0.0 or not normal_gate > 0.0:
        raise ValueError(f"dist_gate {dist_gate} and normal_gate {normal_gate} must be positive")
    return dist_gate, normal_gate


def _iters(iters, min_pairs, show=int):
    """the rule of a loop's ``iters`` / ``min_pairs``, as ints; ``show``: how the error sentence prints the two"""
    if int(iters) < 0 or int(min_pairs) < 6:
        raise ValueError(f"iters {show(iters)} must be >= 0 and min_pairs {show(min_pairs)} >= 6 (the unknowns of a pose)")
    return int(iters), int(min_pairs)


def _call(fns, N, H, W, dev, args):
    """``fns(lib)`` = (an entry point, its workspace query): the entry point on ``args(p)``, then a workspace of that size and the stream"""
    entry, query = fns(cabi.load())
    ws = devargs.workspace(query(N, H, W), dev, query.__name__[len("gdrn_"):])
    cabi.check(entry(*args(cabi.ptr), cabi.ptr(ws), devargs.stream(dev)), entry.__name__[len("gdrn_"):])


def _renders(depth_ren, depth_scene):
    """renders against a scene: (depth_ren [N,H,W] fp32 contiguous, the scene of ``_scene``), on one device and alike in H, W"""
    if not isinstance(depth_ren, torch.Tensor) or depth_ren.device.type != "cuda":
        raise devargs.no_fallback("depth_ren", WHERE)
    if depth_ren.dtype != torch.float32 or depth_ren.dim() != 3:
        raise ValueError("depth_ren must be an fp32 [N, H, W] tensor")
    scene = _scene(depth_scene)
    ren = devargs.device_tensor(depth_ren, None, None, "depth_ren", WHERE)
    if ren.shape[1:] != scene.shape[1:]:
        raise ValueError(f"depth_ren {tuple(ren.shape)} and depth_scene {tuple(scene.shape)} differ in H, W")
    if ren.device != scene.device:
        raise ValueError(f"depth_ren is on {ren.device}, depth_scene on {scene.device}")
    return ren, scene


def _accumulate(fns, depth_ren, depth_scene, frame, K, gates, mask_obs=None):
    """One accumulate pass (``fns``: see ``_call``) on given renders -- with ``mask_obs`` its contour transform first, whose maps the silhouette
    term's pass reads -- and the dict of ``normal_equations`` from the packed systems [N,28]: 21 of A's upper triangle row by row, 6 of b, sq"""
    ren, scene = _renders(depth_ren, depth_scene)
    N, H, W = (int(s) for s in ren.shape)
    dev, F = ren.device, int(scene.shape[0])
    if mask_obs is not None:
        _mask(mask_obs, scene, N)
    K = devargs.per_row_K(devargs.device_tensor(K, torch.float64, (-1, 3, 3), "K", WHERE), N)
    fr, fr_host = devargs.index_vector(frame, N, F, dev, "frame")
    maps = () if mask_obs is None else [contour_transform(mask_obs, scene, fr)[k] for k in ("d2", "nearest")]
    sys = torch.empty(max(N, 1), 28, dtype=torch.float64, device=dev)[:N]
    pairs = torch.empty(max(N, 1), dtype=torch.int32, device=dev)[:N]
    if N > 0:
        _call(fns, N, H, W, dev, lambda p: (p(ren), p(scene), p(fr), fr_host.ctypes.data, F, p(K), *(p(m) for m in maps), N, H, W, *gates, p(sys),
                                            p(pairs)))
    iu = torch.triu_indices(6, 6, device=dev)
    A = torch.zeros(N, 6, 6, dtype=torch.float64, device=dev)
    A[:, iu[0], iu[1]] = sys[:, :21]
    A[:, iu[1], iu[0]] = sys[:, :21]
    return dict(A=A, b=sys[:, 21:27].contiguous(), sq=sys[:, 27].contiguous(), pairs=pairs)


class _Loop:
    """The preamble of a render loop (``icp_refine``, ``icp_refine_sil``, ``depth_align``): the checked tensors, the host index arrays, the
    sizes and the device.  Nothing is loaded or launched here."""

    def __init__(self, meshes, labels, R0, t0, K, depth_scene, frame, mask_obs=None):
        self.meshes = meshes
        self.R, self.t, self.K, self.N = devargs.poses(R0, t0, K, WHERE)
        self.scene = _scene(depth_scene)
        self.dev = self.R.device
        if self.scene.device != self.dev:
            raise ValueError(f"R0 is on {self.dev}, depth_scene on {self.scene.device}")
        self.mask = () if mask_obs is None else (_mask(mask_obs, self.scene, self.N),)
        self.F, self.H, self.W = (int(s) for s in self.scene.shape)
        self.lab, self.lab_host = devargs.index_vector(labels, self.N, meshes.num_classes, self.dev, "labels")
        self.fr, self.fr_host = devargs.index_vector(frame, self.N, self.F, self.dev, "frame")

    def empty(self, dtype):
        return torch.empty(self.N, dtype=dtype, device=self.dev)

    def run(self, fns, R, t, near, far, scalars, outputs):
        """The loop (``fns``: see ``_call``) on the poses ``R``, ``t`` (the caller's copies: in/out for the library): the 22 leading arguments
        in ABI order -- the renderer's own list with the scene and the frames behind N, and the silhouette loop's mask behind F -- then the
        loop's scalars, the scratch render, its outputs, the workspace and the stream"""
        dev, N, H, W = self.dev, self.N, self.H, self.W
        scratch = torch.empty(N, H, W, dtype=torch.float32, device=dev)
        _call(fns, N, H, W, dev, lambda p: (
            *self.meshes.lib_args(dev), p(self.lab), self.lab_host.ctypes.data, p(R), p(t), p(self.K), N, p(self.scene), p(self.fr),
            self.fr_host.ctypes.data, self.F, *(p(m) for m in self.mask), H, W, float(near), float(far),
            *scalars, p(scratch), *(p(o) for o in outputs)))


def normal_equations(depth_ren, depth_scene, frame, K, dist_gate=0.02, normal_gate=0.01):
    """One accumulation on given renders: ``depth_ren`` [N,H,W] fp32 (the model under each estimate's pose, e.g. ``render.render_depth``'s),
    ``depth_scene`` [F,H,W] fp32 (metres, 0 = no measurement), ``frame`` [N] (the frame of each estimate), ``K`` [N,3,3] or [3,3].  Returns a
    dict of device tensors: A [N,6,6] fp64 (symmetric, full), b [N,6], sq [N] fp64 and pairs [N] int32."""
    gates = _gates(dist_gate, normal_gate)
    return _accumulate(lambda lib: (lib.gdrn_icp_accumulate, lib.gdrn_icp_workspace_bytes), depth_ren, depth_scene, frame, K, gates)


def icp_refine(meshes, labels, R0, t0, K, depth_scene, frame, iters=10, dist_gate=0.02, normal_gate=0.01, min_pairs=64, near=render.NEAR,
               far=render.FAR):
    """Refine N estimates against observed depth: ``meshes`` a ``render.MeshTable``, ``labels`` [N] the mesh of each estimate, ``R0`` [N,3,3],
    ``t0`` [N,3], ``K`` [N,3,3] or [3,3] device tensors (fp32 or fp64; model to camera, metres), ``depth_scene`` [F,H,W] fp32 on the device
    (metres, 0 = no measurement), ``frame`` [N] the frame of each estimate.  ``iters`` iterations of render, accumulate and step run on the
    current stream without a host read.  Returns a dict of device tensors: R [N,3,3] and t [N,3] fp64; ok [N] int32 (0: the instance was found
    degenerate -- fewer than ``min_pairs`` pairs or unobservable directions -- and keeps the pose it had); iters_done [N] int32 (steps applied);
    pairs [N] int32 and rms [N] fp64 (metres; NaN without a pair), those of the residual before the instance's last step."""
    dist_gate, normal_gate = _gates(dist_gate, normal_gate)
    iters, min_pairs = _iters(iters, min_pairs)
    c = _Loop(meshes, labels, R0, t0, K, depth_scene, frame)
    R, t = c.R.clone(), c.t.clone()   # in/out for the library; the caller's tensors stay
    out = dict(R=R, t=t, ok=c.empty(torch.int32), iters_done=c.empty(torch.int32), pairs=c.empty(torch.int32), rms=c.empty(torch.float64))
    if c.N > 0:
        c.run(lambda lib: (lib.gdrn_icp_refine, lib.gdrn_icp_workspace_bytes), R, t, near, far, (iters, dist_gate, normal_gate, min_pairs),
              (out["ok"], out["iters_done"], out["pairs"], out["rms"]))
    return out


def _mask(mask_obs, scene, N=None):
    """the observed masks [N,H,W] as uint8 on the scene's device, contiguous"""
    if not isinstance(mask_obs, torch.Tensor) or mask_obs.device.type != "cuda":
        raise devargs.no_fallback("mask_obs", WHERE)
    if mask_obs.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"mask_obs is {mask_obs.dtype}: torch.uint8 or torch.bool (nonzero = object)")
    if mask_obs.dim() != 3 or (N is not None and mask_obs.shape[0] != N):
        raise ValueError(f"mask_obs {tuple(mask_obs.shape)} must be [N, H, W]" + ("" if N is None else f" with N = {N}"))
    if mask_obs.shape[1:] != scene.shape[1:]:
        raise ValueError(f"mask_obs {tuple(mask_obs.shape)} and depth_scene {tuple(scene.shape)} differ in H, W")
    if mask_obs.device != scene.device:
        raise ValueError(f"mask_obs is on {mask_obs.device}, depth_scene on {scene.device}")
    m = devargs.device_tensor(mask_obs, None, None, "mask_obs", WHERE)
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def _sil_args(sil_weight, sil_gate):
    sil_weight, sil_gate = float(sil_weight), float(sil_gate)
    if not (0.0 <= sil_weight < float("inf")) or not sil_gate > 0.0:
        raise ValueError(f"sil_weight {sil_weight} must be finite and >= 0, sil_gate {sil_gate} (pixels) positive")
    return sil_weight, sil_gate


def contour_transform(mask_obs, depth_scene, frame):
    """The contour of observed instance masks and its exact distance transform: ``mask_obs`` [N,H,W] uint8 or bool on the device (nonzero =
    object), ``depth_scene`` [F,H,W] fp32, ``frame`` [N].  A mask pixel with an in-frame 4-neighbour outside the mask is a contour pixel (the
    reference's ``get_edge(mask, bw=1)``: the frame border is no edge) unless such a neighbour holds a nearer observed depth -- an occluder's
    boundary.  Returns a dict of device tensors: d2 [N,H,W] int32 (the squared distance in pixels to the nearest contour pixel of the row's
    mask, exact; INT32_MAX without one), nearest [N,H,W] int32 (y * W + x of that pixel, the smallest on a tie; -1 without one) and contour [N]
    int32 (the number of contour pixels)."""
    scene = _scene(depth_scene)
    m = _mask(mask_obs, scene)
    N, H, W = (int(s) for s in m.shape)
    dev = m.device
    F = int(scene.shape[0])
    fr, fr_host = devargs.index_vector(frame, N, F, dev, "frame")
    out = dict(d2=torch.empty(N, H, W, dtype=torch.int32, device=dev), nearest=torch.empty(N, H, W, dtype=torch.int32, device=dev),
               contour=torch.empty(N, dtype=torch.int32, device=dev))
    lib = cabi.load()
    nbytes = lib.gdrn_sil_workspace_bytes(N, H, W)   # (judges H and W with no rows, too)
    if N == 0:
        cabi.check(min(int(nbytes), 0), "sil_workspace_bytes")
        return out
    ws = devargs.workspace(nbytes, dev, "sil_workspace_bytes")
    p = cabi.ptr
    cabi.check(lib.gdrn_sil_contour_transform(p(m), p(scene), p(fr), fr_host.ctypes.data, F, N, H, W, p(out["d2"]), p(out["nearest"]),
                                              p(out["contour"]), p(ws), devargs.stream(dev)), "sil_contour_transform")
    return out


def silhouette_equations(depth_ren, mask_obs, depth_scene, frame, K, sil_gate=8.0, dist_gate=0.02):
    """One accumulation of the silhouette term on given renders: ``depth_ren`` [N,H,W] fp32, ``mask_obs`` [N,H,W] uint8 or bool,
    ``depth_scene`` [F,H,W] fp32, ``frame`` [N], ``K`` [N,3,3] or [3,3].  A pixel of the render's contour that is not hidden behind a nearer
    observation (by more than ``dist_gate``) and lies within ``sil_gate`` pixels of the observed contour gives two equations: the model point
    must come to lie on the ray of its nearest observed contour pixel.  Returns a dict of device tensors shaped like ``normal_equations``':
    A [N,6,6] fp64 (symmetric, full), b [N,6], sq [N] fp64 (metres squared) and pairs [N] int32 (pixels, two equations each)."""
    _, sil_gate = _sil_args(1.0, sil_gate)
    dist_gate, _ = _gates(dist_gate, 1.0)
    return _accumulate(lambda lib: (lib.gdrn_sil_accumulate, lib.gdrn_sil_workspace_bytes), depth_ren, depth_scene, frame, K, (sil_gate, dist_gate),
                       mask_obs)


def icp_refine_sil(meshes, labels, R0, t0, K, depth_scene, frame, mask_obs, iters=20, sil_weight=1.0, sil_gate=8.0, dist_gate=0.02,
                   normal_gate=0.01, min_pairs=64, near=render.NEAR, far=render.FAR):
    """``icp_refine`` with the silhouette term: the arguments of ``icp_refine`` plus ``mask_obs`` [N,H,W] uint8 or bool on the device, the
    observed instance mask of each estimate in its frame (nonzero = object).  ``contour_transform`` runs once; then ``iters`` times render, the
    depth accumulation, the silhouette accumulation (``silhouette_equations``) and one step from ``depth + sil_weight * silhouette`` with the
    pair counts added, all on the current stream without a host read.  ``sil_weight`` (1.0) and ``sil_gate`` (8 pixels) are parameters: neither
    is measured on real data.  On synthetic plates and cubes weights from 0.25 to 4 end within hundredths of a millimetre of each other, since
    the depth term carries nothing in the directions the contour fixes; the gate must exceed the lateral error of the estimates in pixels.  The
    contour is pixel-quantised: expect a lateral accuracy of a pixel's footprint, not the depth term's.  Returns ``icp_refine``'s dict (pairs
    and rms are the depth term's) plus sil_pairs [N] int32 and sil_rms [N] fp64 (metres; NaN without a pair), the silhouette term's."""
    dist_gate, normal_gate = _gates(dist_gate, normal_gate)
    sil_weight, sil_gate = _sil_args(sil_weight, sil_gate)
    iters, min_pairs = _iters(iters, min_pairs)
    c = _Loop(meshes, labels, R0, t0, K, depth_scene, frame, mask_obs)
    R, t = c.R.clone(), c.t.clone()   # in/out for the library; the caller's tensors stay
    out = dict(R=R, t=t, ok=c.empty(torch.int32), iters_done=c.empty(torch.int32), pairs=c.empty(torch.int32), rms=c.empty(torch.float64),
               sil_pairs=c.empty(torch.int32), sil_rms=c.empty(torch.float64))
    if c.N > 0:
        c.run(lambda lib: (lib.gdrn_icp_refine_sil, lib.gdrn_sil_workspace_bytes), R, t, near, far,
              (iters, dist_gate, normal_gate, min_pairs, sil_weight, sil_gate),
              (out["ok"], out["iters_done"], out["pairs"], out["rms"], out["sil_pairs"], out["sil_rms"]))
    return out


def _align_args(gate, min_pairs, rounds=0):
    gate, min_pairs, rounds = float(gate), int(min_pairs), int(rounds)
    if not gate > 0.0:
        raise ValueError(f"gate {gate} must be positive")
    if min_pairs < 1 or rounds < 0:
        raise ValueError(f"min_pairs {min_pairs} must be >= 1 and rounds {rounds} >= 0")
    return gate, min_pairs, rounds


def depth_offset(depth_ren, depth_scene, frame, gate=0.2, min_pairs=64):
    """The median depth difference of N estimates on given renders: ``depth_ren`` [N,H,W] fp32 (e.g. ``render.render_depth``'s),
    ``depth_scene`` [F,H,W] fp32 (metres, 0 = no measurement), ``frame`` [N].  A pixel is a pair where both depths are positive and
    ``|depth_scene - depth_ren| <= gate``.  Returns a dict of device tensors: offset [N] fp64 (the exact median of ``depth_scene - depth_ren``
    over the pairs; NaN with fewer than ``min_pairs`` pairs), pairs, covered (pixels the render covers) and ok [N] int32."""
    gate, min_pairs, _ = _align_args(gate, min_pairs)
    ren, scene = _renders(depth_ren, depth_scene)
    N, H, W = (int(s) for s in ren.shape)
    dev = ren.device
    F = int(scene.shape[0])
    fr, fr_host = devargs.index_vector(frame, N, F, dev, "frame")
    out = dict(offset=torch.empty(N, dtype=torch.float64, device=dev), pairs=torch.empty(N, dtype=torch.int32, device=dev),
               covered=torch.empty(N, dtype=torch.int32, device=dev), ok=torch.empty(N, dtype=torch.int32, device=dev))
    if N == 0:
        return out
    lib = cabi.load()
    ws = devargs.workspace(lib.gdrn_depth_align_workspace_bytes(N, H, W), dev, "depth_align_workspace_bytes")
    p = cabi.ptr
    cabi.check(lib.gdrn_depth_offset(p(ren), p(scene), p(fr), fr_host.ctypes.data, F, N, H, W, gate, min_pairs, p(out["offset"]), p(out["pairs"]),
                                     p(out["covered"]), p(out["ok"]), p(ws), devargs.stream(dev)), "depth_offset")
    return out


def depth_align(meshes, labels, R0, t0, K, depth_scene, frame, rounds=2, gate=0.2, min_pairs=64, near=render.NEAR, far=render.FAR):
    """Coarse alignment of N estimates along their viewing rays, the step in front of ``icp_refine`` for estimates that are centimetres off
    in depth (an RGB-only pose): ``rounds`` times (a fixed count) the model is rendered under the current pose, the median of
    ``depth_scene - render`` over the pairs is taken (``depth_offset``) and the translation is scaled so that its depth grows by that offset
    and the model origin keeps its image.  The arguments are those of ``icp_refine``; R0 is only read.  ``gate`` must exceed the depth error of
    the estimates and stay below the distance to the background; it is a parameter, and its default of 0.2 m is not measured on real data.
    Returns a dict of device tensors: t [N,3] fp64; ok [N] int32 (0: a round found fewer than ``min_pairs`` pairs -- the instance keeps the
    translation it had and is left alone from then on); pairs, covered [N] int32 and offset [N] fp64 (NaN where ok is 0), those of the
    instance's last evaluated round.  Nothing is read back.  The caller's tensors stay."""
    gate, min_pairs, rounds = _align_args(gate, min_pairs, rounds)
    c = _Loop(meshes, labels, R0, t0, K, depth_scene, frame)
    t = c.t.clone()   # in/out for the library; the caller's tensor stays
    out = dict(t=t, ok=c.empty(torch.int32), pairs=c.empty(torch.int32), covered=c.empty(torch.int32), offset=c.empty(torch.float64))
    if c.N > 0:
        c.run(lambda lib: (lib.gdrn_depth_align, lib.gdrn_depth_align_workspace_bytes), c.R, t, near, far, (rounds, gate, min_pairs),
              (out["ok"], out["pairs"], out["covered"], out["offset"]))
    return out


def refine_rgbd(meshes, labels, R0, t0, K, depth_scene, frame, rounds=2, gate=0.2, align_min_pairs=64, iters=10, dist_gate=0.02,
                normal_gate=0.01, min_pairs=64, near=render.NEAR, far=render.FAR, mask_obs=None, sil_weight=1.0, sil_gate=8.0):
    """``depth_align`` (``rounds``, ``gate``, ``align_min_pairs``), then ``icp_refine`` (``iters``, ``dist_gate``, ``normal_gate``,
    ``min_pairs``) from its translations.  A row that ``depth_align`` could not move (its ok is 0) goes to the ICP with the pose it had.
    With ``mask_obs`` [N,H,W] (the observed instance masks) the second step is ``icp_refine_sil`` with ``sil_weight`` and ``sil_gate``;
    without it the call is what it was before the silhouette term existed.  Returns the second step's dict plus ``align``: the dict of
    ``depth_align``."""
    _gates(dist_gate, normal_gate)   # both steps' scalars are judged before either runs
    _iters(iters, min_pairs, show=lambda v: v)   # (the caller's values as given)
    if mask_obs is not None:
        _sil_args(sil_weight, sil_gate)
        _mask(mask_obs, _scene(depth_scene))
    align = depth_align(meshes, labels, R0, t0, K, depth_scene, frame, rounds=rounds, gate=gate, min_pairs=align_min_pairs, near=near, far=far)
    if mask_obs is None:
        out = icp_refine(meshes, labels, R0, align["t"], K, depth_scene, frame, iters=iters, dist_gate=dist_gate, normal_gate=normal_gate,
                         min_pairs=min_pairs, near=near, far=far)
    else:
        out = icp_refine_sil(meshes, labels, R0, align["t"], K, depth_scene, frame, mask_obs, iters=iters, sil_weight=sil_weight,
                             sil_gate=sil_gate, dist_gate=dist_gate, normal_gate=normal_gate, min_pairs=min_pairs, near=near, far=far)
    out["align"] = align
    return out
