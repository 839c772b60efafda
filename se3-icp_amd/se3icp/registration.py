"""Host-side mirror of the reference's engine interface.

``IterativeSE3Registration`` reproduces the public surface of
``class IterativeSE3Registration`` (include/iterative_SE3_registration.hpp:27-99):
same member names, same constructor defaults (src/iterative_SE3_registration.cpp:334-348),
``setSourceCloud`` / ``setTargetCloud`` (append semantics, ISR.cpp:358-376), the four
``run_*`` methods and the result members ``current_estimated_T_``,
``num_iterations_``, ``num_pure_se3_iterations_``.  Every run goes through the
C-ABI of libse3icp.so to the HIP kernels; nothing here computes registration on
the CPU.

``register_batch`` / ``register_batch_device`` expose the batched path (many scan
pairs in lockstep on one GPU), the MI355X replacement for the serial pair loops of
examples/benchmark_kitti.cpp:120-197 and examples/benchmark_lounge.cpp:154-235.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import threading
import time
from dataclasses import dataclass

import numpy as np

from . import _lib
from .io import read_ply_xyz

_PARAM_FIELDS = {
    # reference member            -> se3icp_params field
    "max_num_iterations_": "max_num_iterations",
    "max_num_se3_iterations_": "max_num_se3_iterations",
    "number_of_nn_for_LRF_": "number_of_nn_for_LRF",
    "mse_": "mse",
    "mse_switch_error_": "mse_switch_error",
    "estimated_overlap_": "estimated_overlap",
    "alpha_rot": "alpha_rot",
    "beta_transl": "beta_transl",
    "scale_preprocessing": "scale_preprocessing",
}


def _as_xyz(cloud) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(cloud, dtype=np.float64))
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"expected an (N, 3) point array, got shape {a.shape}")
    return a


class IterativeSE3Registration:
    """GPU drop-in for the reference class (one object per pair, like the reference)."""

    def __init__(self):
        L = _lib.load()
        object.__setattr__(self, "_L", L)
        object.__setattr__(self, "_h", L.se3icp_registration_new())
        if not self._h:
            raise MemoryError("se3icp_registration_new failed")
        object.__setattr__(self, "_params", L.se3icp_params_of(self._h).contents)
        object.__setattr__(self, "_res", _lib.Result())
        L.se3icp_get_result(self._h, C.byref(self._res))
        # constructor state of the reference (ISR.cpp:334-348); lrf_radius_ is only used by
        # the dead SHOT code path (ISR.cpp:593-594)
        object.__setattr__(self, "lrf_radius_", 0.8)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._L.se3icp_registration_free(h)
            object.__setattr__(self, "_h", None)

    # ---- public config fields (ISR.hpp:80-95)
    def __getattr__(self, name):
        if name in _PARAM_FIELDS:
            return getattr(self._params, _PARAM_FIELDS[name])
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name in _PARAM_FIELDS:
            setattr(self._params, _PARAM_FIELDS[name], value)
        else:
            object.__setattr__(self, name, value)

    # ---- clouds (ISR.cpp:350-376)
    def setSourceCloud(self, cloud):
        pts = read_ply_xyz(cloud) if isinstance(cloud, (str, bytes)) else _as_xyz(cloud)
        _lib.check(self._L.se3icp_set_source_cloud(self._h, pts.ctypes.data_as(C.POINTER(C.c_double)), pts.shape[0]))
        object.__setattr__(self, "_nsrc", getattr(self, "_nsrc", 0) + pts.shape[0])

    def setTargetCloud(self, cloud):
        pts = read_ply_xyz(cloud) if isinstance(cloud, (str, bytes)) else _as_xyz(cloud)
        _lib.check(self._L.se3icp_set_target_cloud(self._h, pts.ctypes.data_as(C.POINTER(C.c_double)), pts.shape[0]))

    def setInitialTransform(self, T):
        """The pose (4x4, source frame -> target frame) every later run_* starts from
        (se3icp_set_initial_transform): current_estimated_T_ is then the composed pose, as
        Open3D's RegistrationICP(..., init) returns it.  None clears."""
        M = None if T is None else _pose_array(T)
        _lib.check(self._L.se3icp_set_initial_transform(self._h, None if M is None else M.ctypes.data_as(_DP)),
                   "setInitialTransform")

    # ---- run methods (ISR.hpp:46-50)
    def _finish(self, rc):
        self._L.se3icp_get_result(self._h, C.byref(self._res))
        if rc in (_lib.ERR_NO_DEVICE, _lib.ERR_HIP, _lib.ERR_OUT_OF_MEMORY, _lib.ERR_EMPTY_CLOUD,
                  _lib.ERR_K_TOO_LARGE, _lib.ERR_INVALID_ARG):
            raise _lib.Se3IcpError(rc)
        return rc

    def run_icp(self, variant_name: str):
        """Vanilla pt2pt / pt2pl / gicp ICP (ISR.cpp:473-552)."""
        return self._finish(self._L.se3icp_run_icp(self._h, variant_name.encode()))

    def run_se3_icp(self, variant_name: str):
        """Proposed SE(3)-ICP, variant in {pt2pt, pt2pl, gicp} (ISR.cpp:555-739)."""
        return self._finish(self._L.se3icp_run_se3_icp(self._h, variant_name.encode()))

    def run_se3_icp_with_cf(self):
        """SE(3)-GICP with depth confidences (ISR.cpp:742-959)."""
        # the C-ABI prints the reference's "### scaling factor = s" line (ISR.cpp:794)
        return self._finish(self._L.se3icp_run_se3_icp_with_cf(self._h))

    def run_se3_pure(self, variant_name: str):
        """SE(3) correspondences only, never switching to R3 (ISR.cpp:962-1127)."""
        # the C-ABI prints the reference's "pure se3 finished" (ISR.cpp:1127)
        return self._finish(self._L.se3icp_run_se3_pure(self._h, variant_name.encode()))

    # ---- registration report (not in the reference: Open3D's RegistrationResult at the final pose)
    def request_report(self, max_correspondence_distance: float = 0.0, per_point: bool = False):
        """Ask the next run_* for a report (``.report``).  per_point: also the final match and
        distance of every source point; call after the source cloud is set."""
        n = getattr(self, "_nsrc", 0)
        idx = np.full(n, -1, np.int32) if per_point else None
        dist = np.zeros(n) if per_point else None
        object.__setattr__(self, "_rep_bufs", (idx, dist))  # kept alive until the run has written them
        opts = _lib.ReportOptions(float(max_correspondence_distance), idx.ctypes.data if per_point else None,
                                  dist.ctypes.data if per_point else None, 0, 0)
        _lib.check(self._L.se3icp_request_report(self._h, C.byref(opts)), "request_report")

    @property
    def report(self):
        """The PairReport of the last run; Se3IcpError (invalid argument) when none was requested."""
        rep = _lib.Report()
        _lib.check(self._L.se3icp_get_report(self._h, C.byref(rep)), "get_report")
        idx, dist = getattr(self, "_rep_bufs", (None, None))
        return _report(rep, idx, dist)

    # ---- results (ISR.hpp:92-98)
    @property
    def current_estimated_T_(self) -> np.ndarray:
        return np.array(self._res.T).reshape(4, 4)

    @property
    def num_iterations_(self) -> int:
        return int(self._res.num_iterations)

    @property
    def num_pure_se3_iterations_(self) -> int:
        return int(self._res.num_pure_se3_iterations)

    @property
    def time_se3_correspondence_search_(self) -> float:
        return float(self._res.time_se3_correspondence_search_ms)

    @property
    def time_before_pure_icp_(self) -> float:
        return float(self._res.time_before_pure_icp_ms)

    @property
    def num_rechecked(self) -> int:
        return int(self._res.num_rechecked)

    @property
    def status(self) -> int:
        return int(self._res.status)


@dataclass
class PairResult:
    T: np.ndarray
    num_iterations: int
    num_pure_se3_iterations: int
    status: int
    num_rechecked: int
    scaling_factor: float
    time_setup_ms: float
    time_loop_ms: float
    time_nn_ms: float
    time_before_pure_icp_ms: float


def _results(res, n) -> list[PairResult]:
    out = []
    for i in range(n):
        r = res[i]
        out.append(PairResult(np.array(r.T).reshape(4, 4), int(r.num_iterations), int(r.num_pure_se3_iterations),
                              int(r.status), int(r.num_rechecked), float(r.scaling_factor), float(r.time_setup_ms),
                              float(r.time_loop_ms), float(r.time_se3_correspondence_search_ms),
                              float(r.time_before_pure_icp_ms)))
    return out


def cli_params(**overrides) -> _lib.Params:
    """Parameter overrides of examples/run_registration_method.cpp:38-42."""
    p = _lib.default_params(estimated_overlap=1.0, max_num_se3_iterations=10, mse=1e-5, mse_switch_error=5e-5,
                            number_of_nn_for_LRF=90)
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def kitti_params(**overrides) -> _lib.Params:
    """SE(3) parameters of examples/benchmark_kitti.cpp:133-148."""
    p = _lib.default_params(estimated_overlap=0.7, max_num_se3_iterations=10, mse=1e-7, mse_switch_error=5e-7,
                            number_of_nn_for_LRF=90)
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def lounge_params(**overrides) -> _lib.Params:
    """Parameters of examples/benchmark_lounge.cpp:183-189."""
    p = _lib.default_params(estimated_overlap=0.75, max_num_se3_iterations=10, mse_switch_error=5e-5,
                            number_of_nn_for_LRF=90)
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


# ---- marshalling shared by the register_* functions below
_DP = C.POINTER(C.c_double)


def _pair_args(pairs):
    """(n, the four pointer / size arguments of a host entry, the source sizes, the arrays
    those point into: the caller holds them until the call has returned)."""
    srcs = [_as_xyz(s) for s, _ in pairs]
    tgts = [_as_xyz(t) for _, t in pairs]
    n = len(pairs)
    counts = [a.shape[0] for a in srcs]
    args = ((_DP * n)(*[a.ctypes.data_as(_DP) for a in srcs]), (C.c_int64 * n)(*counts),
            (_DP * n)(*[a.ctypes.data_as(_DP) for a in tgts]), (C.c_int64 * n)(*[a.shape[0] for a in tgts]))
    return n, args, counts, (srcs, tgts)


def _offset_args(src_ptr: int, src_off, tgt_ptr: int, tgt_off):
    """(n, the four pointer / offset arguments of a *_device entry)."""
    n = len(src_off) - 1
    return n, (C.c_void_p(src_ptr), (C.c_int64 * (n + 1))(*[int(x) for x in src_off]),
               C.c_void_p(tgt_ptr), (C.c_int64 * (n + 1))(*[int(x) for x in tgt_off]))


def _cloud_args(clouds):
    """(the (N, 3) arrays of a cloud set, the count / pointer / size arguments of a graph entry)."""
    cl = [_as_xyz(c) for c in clouds]
    nc = len(cl)
    return cl, (nc, (_DP * max(nc, 1))(*[a.ctypes.data_as(_DP) for a in cl]),
                (C.c_int64 * max(nc, 1))(*[a.shape[0] for a in cl]))


def _outputs(n):
    """Result and report arrays of n slots (one at least: the C side is never handed an empty array)."""
    return (_lib.Result * max(1, n))(), (_lib.Report * max(1, n))()


def _params_ref(params):
    return C.byref(params or _lib.default_params())


def _stream_arg(stream: int):
    return C.c_void_p(stream) if stream else None


def _registered(rc: int, what: str) -> None:
    """Raise unless the call ran (a non-finite pose is a pair's status, not the call's failure)."""
    if rc not in (_lib.OK, _lib.ERR_NONFINITE):
        raise _lib.Se3IcpError(rc, what)


def _pose_array(T) -> np.ndarray:
    M = np.ascontiguousarray(np.asarray(T, dtype=np.float64))
    if M.shape != (4, 4):
        raise ValueError(f"expected a 4x4 pose, got shape {M.shape}")
    return M


def _init_array(init, n_edges: int):
    """The T_init argument of the *_init entries: None (no edge is posed), or the (n_edges, 4, 4)
    array of `init`, a sequence of 4x4 poses or Nones (None: the identity, "no pose")."""
    if init is None:
        return None
    init = list(init)
    if len(init) != n_edges:
        raise ValueError(f"init has {len(init)} entries for {n_edges} edges")
    if all(t is None for t in init):
        return None
    return np.ascontiguousarray(np.stack([np.eye(4) if t is None else _pose_array(t) for t in init]))


def register_batch(pairs, method: str, params: _lib.Params | None = None, device: int = 0,
                   init=None) -> list[PairResult]:
    """Register [(src (N,3), tgt (M,3)), ...] in lockstep on one GPU (host buffers).  init: one
    4x4 initial pose (or None) per pair; the call then goes through the graph entry with every
    cloud distinct (register_graph(init=...))."""
    if _init_array(init, len(pairs)) is not None:
        clouds = [c for pair in pairs for c in pair]
        return register_graph(clouds, [(2 * p, 2 * p + 1) for p in range(len(pairs))], method, params, device,
                              init=init)
    n, args, _, _keep = _pair_args(pairs)
    res, _ = _outputs(n)
    _registered(_lib.load().se3icp_register_batch(device, n, *args, _lib.method_id(method), _params_ref(params), res),
                "register_batch")
    return _results(res, n)


def register_batch_device(src_ptr: int, src_off, tgt_ptr: int, tgt_off, method: str,
                          params: _lib.Params | None = None, device: int = 0, stream: int = 0) -> list[PairResult]:
    """Register pairs whose clouds are already in HBM.

    src_ptr/tgt_ptr: device addresses of the concatenated AoS float64 xyz arrays
    (e.g. ``torch_tensor.data_ptr()``); src_off/tgt_off: n_pairs+1 point offsets.
    """
    n, args = _offset_args(src_ptr, src_off, tgt_ptr, tgt_off)
    res, _ = _outputs(n)
    _registered(_lib.load().se3icp_register_batch_device(device, n, *args, _lib.method_id(method), _params_ref(params),
                                                         res, _stream_arg(stream)), "register_batch_device")
    return _results(res, n)


class DeviceBatchRunner:
    """``register_batch_device`` for repeated calls on the same clouds (benchmark loops):
    the ctypes arguments are built once, each ``run(slot)`` is one C-ABI call writing into
    preallocated result / kernel-time buffers, and the conversion to ``PairResult`` happens
    later (``results(slot)``, ``kernel_times(slot)``), outside the caller's timed region."""

    _KT_KEYS = ["nn_se3_ms", "nn_r3_ms", "recheck_ms", "trim_ms", "reduce_ms", "setup_ms", "nn_se3_launches",
                "nn_r3_launches", "se3_dist_evals", "se3_box_tests", "r3_dist_evals", "r3_box_tests",
                "lrf_ms", "lrf_queries", "lrf_leaves", "lrf_merges", "lrf_box_tests", "lrf_candidates",
                "nn_prep_ms", "se3_queries", "se3_searched", "r3_queries", "r3_searched", "lrf_fallback",
                "se3_useful_evals", "r3_useful_evals"]

    def __init__(self, src_ptr: int, src_off, tgt_ptr: int, tgt_off, method: str,
                 params: _lib.Params | None = None, device: int = 0, slots: int = 1):
        self._L = _lib.load()
        self.n = len(src_off) - 1
        self._dev = device
        self._so = (C.c_int64 * (self.n + 1))(*[int(x) for x in src_off])
        self._to = (C.c_int64 * (self.n + 1))(*[int(x) for x in tgt_off])
        self._src = C.c_void_p(src_ptr)
        self._tgt = C.c_void_p(tgt_ptr)
        self._mid = _lib.method_id(method)
        self._params = params or _lib.default_params()
        self._pref = C.byref(self._params)
        self._res = [(_lib.Result * self.n)() for _ in range(max(1, slots))]
        self._kt = [(C.c_double * len(self._KT_KEYS))() for _ in range(max(1, slots))]

    def run(self, slot: int = 0) -> None:
        rc = self._L.se3icp_register_batch_device(self._dev, self.n, self._src, self._so, self._tgt, self._to,
                                                  self._mid, self._pref, self._res[slot], None)
        if rc not in (_lib.OK, _lib.ERR_NONFINITE):
            raise _lib.Se3IcpError(rc, "register_batch_device")
        self._L.se3icp_last_kernel_times_n(self._dev, self._kt[slot], len(self._KT_KEYS))

    def results(self, slot: int = 0) -> list[PairResult]:
        return _results(self._res[slot], self.n)

    def kernel_times(self, slot: int = 0) -> dict:
        return dict(zip(self._KT_KEYS, list(self._kt[slot])))


class PipelinedBatchRunner:
    """Consecutive batches with ``in_flight`` of them on the GPU at once: one engine slot per
    in-flight call (``device | slot << 8``: own stream and buffers) and a
    host thread per slot taking the next step index until ``steps`` calls are done (ctypes
    releases the GIL during the C-ABI call).  A call is latency-bound over much of its loop
    (small per-iteration grids, host-visible phase switches) while its setup is not, so a
    second call in flight fills what the first leaves idle.  Every call registers the same
    clouds and returns bitwise the results of a lone call (per-slot engines share nothing).

    runner_factory(slot) -> an object with run(i), results(i), kernel_times(i) over ``steps``
    result buffers (DeviceBatchRunner; tests pass stand-ins)."""

    def __init__(self, runner_factory, in_flight: int = 2, steps: int = 1):
        self._lock = threading.Lock()
        self.in_flight = max(1, int(in_flight))
        self.steps = max(1, int(steps))
        self._runners = [runner_factory(k) for k in range(self.in_flight)]
        self._owner = [-1] * self.steps
        self._wall = [0.0] * self.steps  # each call's wall time (s): its latency with the others in flight

    def warm(self) -> None:
        """One untimed call per slot (its buffers and code), into result buffer 0."""
        for r in self._runners:
            r.run(0)

    def run_steps(self, steps: int | None = None) -> None:
        n = self.steps if steps is None else min(int(steps), self.steps)
        nxt = [0]
        err: list[BaseException] = []

        def worker(k: int) -> None:
            while True:
                with self._lock:
                    s = nxt[0]
                    if s >= n or err:
                        return
                    nxt[0] = s + 1
                    self._owner[s] = k
                try:
                    t0 = time.perf_counter()
                    self._runners[k].run(s)
                    self._wall[s] = time.perf_counter() - t0
                except BaseException as e:  # noqa: BLE001 (re-raised by the caller's thread)
                    with self._lock:
                        err.append(e)
                    return

        if self.in_flight == 1:
            for s in range(n):
                self._owner[s] = 0
                t0 = time.perf_counter()
                self._runners[0].run(s)
                self._wall[s] = time.perf_counter() - t0
            return
        th = [threading.Thread(target=worker, args=(k,)) for k in range(self.in_flight)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        if err:
            raise err[0]

    def owner(self, s: int) -> int:
        return self._owner[s]

    def call_seconds(self, s: int) -> float:
        """Wall time of call s (from its start to its return, others in flight beside it)."""
        return self._wall[s]

    def results(self, s: int) -> list[PairResult]:
        return self._runners[self._owner[s]].results(s)

    def kernel_times(self, s: int) -> dict:
        return self._runners[self._owner[s]].kernel_times(s)


@contextlib.contextmanager
def _armed_trace(device: int, slot: int, n_src: int, max_iters: int):
    """Arm the per-iteration record of result slot `slot` (a source of n_src points) for the one
    registration call made inside the block; the dict it yields holds, after the block, the
    recorded arrays cut to the recorded iterations."""
    L = _lib.load()
    tr = {"corr_idx": np.full((max_iters, n_src), -1, np.int32), "corr_dist": np.zeros((max_iters, n_src), np.float32),
          "trim_key": np.zeros(max_iters, np.uint64), "T": np.zeros((max_iters, 4, 4)), "mse": np.zeros(max_iters),
          "phase": np.zeros(max_iters, np.int32)}
    t = _lib.Trace(slot, max_iters, tr["corr_idx"].ctypes.data_as(C.POINTER(C.c_int32)),
                   tr["corr_dist"].ctypes.data_as(C.POINTER(C.c_float)),
                   tr["trim_key"].ctypes.data_as(C.POINTER(C.c_uint64)), tr["T"].ctypes.data_as(_DP),
                   tr["mse"].ctypes.data_as(_DP), tr["phase"].ctypes.data_as(C.POINTER(C.c_int32)), 0, 0)
    _lib.check(L.se3icp_set_trace(device, C.byref(t)), "set_trace")
    trace = {}
    try:
        yield trace
    finally:
        L.se3icp_set_trace(device, None)
    n = int(t.iters_recorded)
    trace.update({k: v[:n] for k, v in tr.items()})


@contextlib.contextmanager
def setup_record(pair: int, n_src: int, n_tgt: int, device: int = 0):
    """Arm the setup record (se3icp_set_setup_record) of result slot `pair` -- a source of n_src
    and a target of n_tgt points -- for the one registration call made inside the block, through
    any register_* entry (host, device, stream, sweep: slot v * n_pairs + p, graph: the edge).
    The dict it yields holds, after the block, per side "src" / "tgt" a dict of
    xyz (n, 3), rows (n, 12), normals (n, 3), conf (n,) -- None where the method does not produce
    the array -- and the setup scalars norm_center, norm_scale, f32_center, alpha, beta, n."""
    L = _lib.load()
    rec = _lib.SetupRecord()
    rec.pair = int(pair)
    bufs = {}
    for name, n in (("src", int(n_src)), ("tgt", int(n_tgt))):
        side = getattr(rec, name)
        bufs[name] = {"xyz": np.zeros((n, 3)), "rows": np.zeros((n, 12)), "normals": np.zeros((n, 3)),
                      "conf": np.zeros(n)}
        for key, a in bufs[name].items():
            setattr(side, key, a.ctypes.data_as(_DP))
        side.cap = n
    _lib.check(L.se3icp_set_setup_record(device, C.byref(rec)), "set_setup_record")
    out = {}
    try:
        yield out
    finally:
        L.se3icp_set_setup_record(device, None)
    if not rec.recorded:
        raise _lib.Se3IcpError(_lib.ERR_INTERNAL, "the call inside the block took no setup record")
    bits = {"xyz": _lib.SETUP_XYZ, "rows": _lib.SETUP_ROWS, "normals": _lib.SETUP_NORMALS, "conf": _lib.SETUP_CONF}
    for name in ("src", "tgt"):
        side = getattr(rec, name)
        n = int(side.n)
        d = {key: (bufs[name][key][:n] if side.written & bit else None) for key, bit in bits.items()}
        d.update(n=n, norm_center=np.array(side.norm_center[:]), norm_scale=float(side.norm_scale),
                 f32_center=np.array(side.f32_center[:]), alpha=float(side.alpha), beta=float(side.beta))
        out[name] = d


_TREE_BITS = {"perm": _lib.TREE_PERM, "pos": _lib.TREE_POS, "vec": _lib.TREE_VEC, "tvec": _lib.TREE_TVEC,
              "tvec64": _lib.TREE_TVEC64, "tpt64": _lib.TREE_TPT64, "lo": _lib.TREE_BOXES, "hi": _lib.TREE_BOXES}


@contextlib.contextmanager
def tree_record(pair: int, n_src: int, n_tgt: int, device: int = 0, n_max: int | None = None):
    """Arm the tree record (se3icp_set_tree_record) of result slot `pair` -- a source of n_src and
    a target of n_tgt points -- for the one call made inside the block: any register_* entry, or
    nearest_neighbors / nearest_neighbors_sequence (pair 0: the queries and the data).  n_max: the
    largest cloud of the call (default: the larger of the two), which sets the trees' depth and so
    the room the boxes need.  The dict it yields holds, after the block, under "src3", "tgt3",
    "src12", "tgt12" None for a tree the call did not build, otherwise a dict of the scalars n, D,
    L, nnodes, G, H, role (-1: built, else the donor's cloud slot), written, and the arrays perm
    (n,), pos (n,), vec (n, D), tvec (n, D), tvec64 (n, 3), tpt64 (n, 4), lo / hi (nnodes, D) --
    None where the build does not produce the array for that tree."""
    L = _lib.load()
    rec = _lib.TreeRecord()
    rec.pair = int(pair)
    n_max = max(int(n_src), int(n_tgt), int(n_max or 0), 1)
    depth = 0
    while (n_max + (1 << depth) - 1) >> depth > 64:  # tree_depth_for (tree.hpp)
        depth += 1
    nodes = (2 << depth) - 1
    ptr = {np.dtype(np.int32): C.POINTER(C.c_int32), np.dtype(np.float32): C.POINTER(C.c_float),
           np.dtype(np.float64): _DP}
    bufs = {}
    for name, n, D in (("src3", int(n_src), 3), ("tgt3", int(n_tgt), 3), ("src12", int(n_src), 12),
                       ("tgt12", int(n_tgt), 12)):
        side = getattr(rec, name)
        bufs[name] = {"perm": np.zeros(n, np.int32), "pos": np.zeros(n, np.int32), "vec": np.zeros((n, D), np.float32),
                      "tvec": np.zeros((n, D), np.float32), "tvec64": np.zeros((n, 3)), "tpt64": np.zeros((n, 4)),
                      "lo": np.zeros((nodes, D), np.float32), "hi": np.zeros((nodes, D), np.float32)}
        for key, a in bufs[name].items():
            setattr(side, key, a.ctypes.data_as(ptr[a.dtype]))
        side.cap = n
        side.node_cap = nodes
    _lib.check(L.se3icp_set_tree_record(device, C.byref(rec)), "set_tree_record")
    out = {}
    try:
        yield out
    finally:
        L.se3icp_set_tree_record(device, None)
    if not rec.recorded:
        raise _lib.Se3IcpError(_lib.ERR_INTERNAL, "the call inside the block took no tree record")
    for name in bufs:
        side = getattr(rec, name)
        if not side.exists:
            out[name] = None
            continue
        n, nn = int(side.n), int(side.nnodes)
        d = {key: ((a[:nn] if key in ("lo", "hi") else a[:n]) if side.written & _TREE_BITS[key] else None)
             for key, a in bufs[name].items()}
        d.update(n=n, D=int(side.D), L=int(side.L), nnodes=nn, G=int(side.G), H=int(side.H), role=int(side.role),
                 written=int(side.written))
        out[name] = d


def register_batch_traced(pairs, method: str, params: _lib.Params | None = None, pair: int = 0,
                          max_iters: int = 160, device: int = 0):
    """register_batch with the per-iteration record of one pair (se3icp_set_trace): the
    pre-trim correspondence set (target index, float distance) of every iteration, the
    trimmed rejector's cut, the pose and the MSE after it and the phase it ran in.
    Returns (results, trace dict with arrays cut to the recorded iterations)."""
    with _armed_trace(device, pair, _as_xyz(pairs[pair][0]).shape[0], max_iters) as trace:
        res = register_batch(pairs, method, params, device)
    return res, trace


# ---- parameter sweeps (the outer loop of the reference's benchmark drivers)
def alpha_grid() -> list[float]:
    """The 47 values of alpha_rot the reference's drivers sweep: makeHybridLGrid()
    (examples/benchmark_kitti.cpp:354-384, the same in the lounge, synthetic and pure-SE(3)
    drivers), with its double arithmetic: 0, i * 0.01 (i = 1..10), i * 0.1 (i = 2..10),
    1.0 + i * 0.5 (i = 0..8), the literal tail, sorted, duplicates removed."""
    g = [0.0]
    g += [i * 0.01 for i in range(1, 11)]
    g += [i * 0.1 for i in range(2, 11)]
    g += [1.0 + i * 0.5 for i in range(0, 9)]
    g += [5.0, 7.0, 10.0, 15.0, 25.0, 50.0, 60.0, 70.0, 80.0, 90.0, 100.0, 200.0, 300.0, 400.0, 500.0, 600.0, 700.0,
          800.0, 900.0, 1000.0]
    return sorted(set(g))


def _copy_params(p: _lib.Params) -> _lib.Params:
    q = _lib.Params()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(_lib.Params))
    return q


def sweep_params(base: _lib.Params | None = None, **lists) -> list[_lib.Params]:
    """The variants of a sweep: copies of ``base`` with the listed fields replaced, entry i
    taking element i of every list (lists of one length), e.g.
    ``sweep_params(kitti_params(), alpha_rot=alpha_grid())``."""
    base = base or _lib.default_params()
    lens = {len(v) for v in lists.values()}
    if len(lens) != 1:
        raise ValueError("sweep_params: give at least one list, all of one length")
    fields = {f[0] for f in _lib.Params._fields_}
    out = []
    for i in range(lens.pop()):
        q = _copy_params(base)
        for k, vals in lists.items():
            if k not in fields or k.startswith("_"):
                raise ValueError(f"sweep_params: no parameter {k!r}")
            setattr(q, k, vals[i])
        out.append(q)
    return out


def _variant_array(variants):
    """(the number of variants, their array; NULL for none)."""
    nv = len(variants)
    arr = (_lib.Params * nv)()
    for i, p in enumerate(variants):
        C.memmove(C.byref(arr, i * C.sizeof(_lib.Params)), C.byref(p), C.sizeof(_lib.Params))
    return nv, (arr if nv else None)


def _sweep_results(res, nv, n) -> list[list[PairResult]]:
    flat = _results(res, nv * n)
    return [flat[v * n:(v + 1) * n] for v in range(nv)]


def register_sweep(pairs, method: str, variants, device: int = 0, max_group: int = 0) -> list[list[PairResult]]:
    """Register every pair under every parameter set of ``variants`` (a list of Params that
    share number_of_nn_for_LRF and scale_preprocessing) with one shared setup; result
    ``[v][p]`` is bitwise what ``register_batch(pairs, method, variants[v])[p]`` returns.
    max_group: variants registered in lockstep at once (0: the engine's choice)."""
    n, args, _, _keep = _pair_args(pairs)
    nv, var = _variant_array(variants)
    res, _ = _outputs(nv * n)
    _registered(_lib.load().se3icp_register_sweep(device, n, *args, _lib.method_id(method), nv, var, max_group, res),
                "register_sweep")
    return _sweep_results(res, nv, n)


def register_sweep_device(src_ptr: int, src_off, tgt_ptr: int, tgt_off, method: str, variants, device: int = 0,
                          stream: int = 0, max_group: int = 0) -> list[list[PairResult]]:
    """register_sweep for clouds already in HBM (arguments as register_batch_device)."""
    n, args = _offset_args(src_ptr, src_off, tgt_ptr, tgt_off)
    nv, var = _variant_array(variants)
    res, _ = _outputs(nv * n)
    _registered(_lib.load().se3icp_register_sweep_device(device, n, *args, _lib.method_id(method), nv, var, max_group,
                                                         res, _stream_arg(stream)), "register_sweep_device")
    return _sweep_results(res, nv, n)


def register_sweep_traced(pairs, method: str, variants, variant: int = 0, pair: int = 0, max_iters: int = 160,
                          device: int = 0, max_group: int = 0):
    """register_sweep with the per-iteration record of pair ``pair`` under variant ``variant``
    (see register_batch_traced).  Returns (results, trace dict)."""
    with _armed_trace(device, variant * len(pairs) + pair, _as_xyz(pairs[pair][0]).shape[0], max_iters) as trace:
        res = register_sweep(pairs, method, variants, device, max_group)
    return res, trace


# ---- registration reports (fitness, RMSE, information matrix and final matches per pair)
@dataclass
class PairReport:
    fitness: float
    inlier_rmse: float
    information: np.ndarray          # (6, 6), rotation first
    final_mse: float
    final_mse_change: float
    n_inliers: int
    switched: int
    stop_reason: int                 # _lib.STOP_*
    corr_idx: np.ndarray | None = None   # (n_src,) int32: the final match of every source point
    corr_dist: np.ndarray | None = None  # (n_src,) its distance, caller's units

    @property
    def stop_reason_name(self) -> str:
        return _lib.STOP_REASONS[self.stop_reason]


def _report(r, idx=None, dist=None) -> PairReport:
    return PairReport(float(r.fitness), float(r.inlier_rmse), np.array(r.information).reshape(6, 6), float(r.final_mse),
                      float(r.final_mse_change), int(r.n_inliers), int(r.switched), int(r.stop_reason), idx, dist)


def _report_options(max_correspondence_distance: float, idx_ptr=None, dist_ptr=None, on_device=False):
    return _lib.ReportOptions(float(max_correspondence_distance), idx_ptr, dist_ptr, 1 if on_device else 0, 0)


def _per_point_options(max_correspondence_distance: float, counts, per_point: bool):
    """(report options, the per-point match and distance buffers they point at -- None without
    per_point) for pairs of `counts` source points."""
    idx = np.full(sum(counts), -1, np.int32) if per_point else None
    dist = np.zeros(sum(counts)) if per_point else None
    return _report_options(max_correspondence_distance, idx.ctypes.data if per_point else None,
                           dist.ctypes.data if per_point else None), idx, dist


def _pair_reports(rep, counts, idx=None, dist=None) -> list[PairReport]:
    """One PairReport per pair, each with its own stretch of the per-point buffers (if any)."""
    out, at = [], 0
    for i, n in enumerate(counts):
        out.append(_report(rep[i], None if idx is None else idx[at:at + n], None if dist is None else dist[at:at + n]))
        at += n
    return out


def register_batch_report(pairs, method: str, params: _lib.Params | None = None, device: int = 0,
                          max_correspondence_distance: float = 0.0, per_point: bool = False):
    """register_batch plus a PairReport per pair, evaluated at the final pose: returns
    (results, reports); the results are bitwise register_batch's.  A distance <= 0 or inf makes
    every point an inlier.  per_point: also the final match and its distance of every source
    point (PairReport.corr_idx / corr_dist)."""
    n, args, counts, _keep = _pair_args(pairs)
    res, rep = _outputs(n)
    opts, idx, dist = _per_point_options(max_correspondence_distance, counts, per_point)
    _registered(_lib.load().se3icp_register_batch_report(device, n, *args, _lib.method_id(method), _params_ref(params),
                                                         res, C.byref(opts), rep), "register_batch_report")
    return _results(res, n), _pair_reports(rep, counts, idx, dist)


def register_batch_report_device(src_ptr: int, src_off, tgt_ptr: int, tgt_off, method: str,
                                 params: _lib.Params | None = None, device: int = 0, stream: int = 0,
                                 max_correspondence_distance: float = 0.0, corr_idx_ptr: int = 0,
                                 corr_dist_ptr: int = 0, outputs_on_device: bool = True):
    """register_batch_device plus reports: returns (results, reports).  corr_idx_ptr /
    corr_dist_ptr: optional addresses of int32 / float64 buffers of sum(n_src) entries (pair p
    at src_off[p] - src_off[0]) that receive the final matches -- device addresses (e.g.
    ``torch_tensor.data_ptr()``) when outputs_on_device, host addresses otherwise."""
    n, args = _offset_args(src_ptr, src_off, tgt_ptr, tgt_off)
    res, rep = _outputs(n)
    opts = _report_options(max_correspondence_distance, corr_idx_ptr or None, corr_dist_ptr or None, outputs_on_device)
    _registered(_lib.load().se3icp_register_batch_report_device(device, n, *args, _lib.method_id(method),
                                                                _params_ref(params), res, _stream_arg(stream),
                                                                C.byref(opts), rep), "register_batch_report_device")
    return _results(res, n), [_report(rep[i]) for i in range(n)]


def _sweep_reports(rep, nv, n):
    return [[_report(rep[v * n + p]) for p in range(n)] for v in range(nv)]


def register_sweep_report(pairs, method: str, variants, device: int = 0, max_group: int = 0,
                          max_correspondence_distance: float = 0.0):
    """register_sweep plus reports: returns (results[v][p], reports[v][p]), e.g. to pick the
    alpha_rot of a sweep by fitness where there is no ground truth."""
    n, args, _, _keep = _pair_args(pairs)
    nv, var = _variant_array(variants)
    res, rep = _outputs(nv * n)
    opts = _report_options(max_correspondence_distance)
    _registered(_lib.load().se3icp_register_sweep_report(device, n, *args, _lib.method_id(method), nv, var, max_group,
                                                         res, C.byref(opts), rep), "register_sweep_report")
    return _sweep_results(res, nv, n), _sweep_reports(rep, nv, n)


def register_sweep_report_device(src_ptr: int, src_off, tgt_ptr: int, tgt_off, method: str, variants, device: int = 0,
                                 stream: int = 0, max_group: int = 0, max_correspondence_distance: float = 0.0):
    """register_sweep_report for clouds already in HBM."""
    n, args = _offset_args(src_ptr, src_off, tgt_ptr, tgt_off)
    nv, var = _variant_array(variants)
    res, rep = _outputs(nv * n)
    opts = _report_options(max_correspondence_distance)
    _registered(_lib.load().se3icp_register_sweep_report_device(device, n, *args, _lib.method_id(method), nv, var,
                                                                max_group, res, _stream_arg(stream), C.byref(opts),
                                                                rep), "register_sweep_report_device")
    return _sweep_results(res, nv, n), _sweep_reports(rep, nv, n)


# ---- stage entry points (one per reference function on the hot path)
# ---- cloud graphs (pairs over a shared set of clouds, each cloud set up once)
def sequence_edges(n: int) -> list[tuple[int, int]]:
    """The edges of the reference's odometry drivers over n scans: scan i+1 registered onto
    scan i (examples/benchmark_kitti.cpp:120-131), as (source, target) cloud indices."""
    return [(i + 1, i) for i in range(max(0, int(n) - 1))]


def expand_edges(clouds, edges):
    """The (source, target) pair list register_batch takes for `edges` over `clouds`."""
    return [(clouds[int(s)], clouds[int(t)]) for s, t in edges]


def _edge_arrays(edges):
    n = len(edges)
    es = (C.c_int32 * max(n, 1))(*[int(s) for s, _ in edges])
    et = (C.c_int32 * max(n, 1))(*[int(t) for _, t in edges])
    return n, es, et


def edge_inits(poses, edges) -> list[np.ndarray]:
    """What a loop-closure caller passes as `init`: for absolute poses world_T_cloud (4x4 each) the
    relative pose inv(P_t) @ P_s of every (s, t) of `edges`, with the rigid inverse
    [R^T | -R^T t], in float64.  (A convenience: its arithmetic is not part of the bitwise
    contract of register_graph(init=...), which starts at the poses it is handed.)"""
    out = []
    for s, t in edges:
        Ps, Pt = _pose_array(poses[int(s)]), _pose_array(poses[int(t)])
        inv = np.eye(4)
        inv[:3, :3] = Pt[:3, :3].T
        inv[:3, 3] = -(Pt[:3, :3].T @ Pt[:3, 3])
        M = inv @ Ps
        M[3] = (0.0, 0.0, 0.0, 1.0)
        out.append(M)
    return out


def transform_points(T, xyz) -> np.ndarray:
    """apply_pose(T, p) for every point of an (N, 3) array, on the host, in the engine's pinned
    arithmetic (se3icp_transform_points): bitwise what register_graph(init=...) registers."""
    pts, M = _as_xyz(xyz), _pose_array(T)
    out = np.empty_like(pts)
    _lib.check(_lib.load().se3icp_transform_points(M.ctypes.data_as(_DP), pts.ctypes.data_as(_DP), pts.shape[0],
                                                   out.ctypes.data_as(_DP)), "transform_points")
    return out


def transform_device(xyz_ptr: int, off, poses, out_ptr: int | None = None, device: int = 0, stream: int = 0) -> None:
    """One pose per cloud applied to clouds resident in HBM, all in one launch
    (se3icp_transform_device): xyz_ptr / off as register_graph_device, poses n_clouds 4x4 arrays,
    out_ptr a device buffer laid out as the input (None: in place)."""
    nc = len(off) - 1
    co = (C.c_int64 * (max(nc, 0) + 1))(*[int(x) for x in off])
    M = np.ascontiguousarray(np.stack([_pose_array(t) for t in poses])) if nc > 0 else np.zeros((1, 4, 4))
    if nc > 0 and M.shape[0] != nc:
        raise ValueError(f"{M.shape[0]} poses for {nc} clouds")
    _lib.check(_lib.load().se3icp_transform_device(int(device), nc, C.c_void_p(xyz_ptr), co, M.ctypes.data_as(_DP),
                                                   C.c_void_p(xyz_ptr if out_ptr is None else out_ptr),
                                                   _stream_arg(stream)), "transform_device")


def set_pose_seeding(mode: int, device: int = 0) -> None:
    """Whether the posed copies of a cloud seed each other's neighbour selection on the engine
    behind `device` (se3icp_set_pose_seeding): 0 across poses (the default), 1 within one (cloud,
    pose) only.  Results are bitwise the same; last_init_stats() describes the last call."""
    _lib.check(_lib.load().se3icp_set_pose_seeding(int(device), int(mode)), "set_pose_seeding")


def last_init_stats(device: int = 0) -> dict:
    """Initial-pose counters of the last graph call on `device` (se3icp_last_init_stats)."""
    out = (C.c_int64 * len(_lib.INIT_STATS))()
    _lib.check(_lib.load().se3icp_last_init_stats(int(device), out, len(_lib.INIT_STATS)), "last_init_stats")
    return {k: int(out[i]) for i, k in enumerate(_lib.INIT_STATS)}


def register_graph(clouds, edges, method: str, params: _lib.Params | None = None, device: int = 0,
                   sharing: int = 0, voxel_size: float | None = None, init=None) -> list[PairResult]:
    """Register clouds[s] onto clouds[t] for every (s, t) of `edges`: result p is bitwise
    register_batch's for that pair, but every distinct cloud is uploaded and ingested once and
    set up once per normalization it takes part in (se3icp_register_graph).  sharing: 0 the
    engine's choice, 1 .. 3 see include/se3icp.h.  voxel_size: the clouds are raw scans; each is
    uploaded once, voxel-downsampled in HBM (voxel_downsample_device) and the result registered
    by the device entry -- bitwise register_graph of the clouds voxel_downsample returns.
    init: one 4x4 initial pose (source frame -> target frame) or None per edge
    (se3icp_register_graph_init): result p is bitwise the plain call's for
    (transform_points(init[p], source), target) except T, which is the composed pose."""
    if voxel_size is not None:
        return _register_graph_voxel(clouds, edges, method, params, device, sharing, float(voxel_size), init)
    _keep, cargs = _cloud_args(clouds)
    n, es, et = _edge_arrays(edges)
    res, _ = _outputs(n)
    T0 = _init_array(init, n)
    if T0 is not None:
        _registered(_lib.load().se3icp_register_graph_init(device, *cargs, n, es, et, T0.ctypes.data_as(_DP),
                                                           _lib.method_id(method), _params_ref(params), int(sharing),
                                                           res, None, None), "register_graph_init")
        return _results(res, n)
    _registered(_lib.load().se3icp_register_graph(device, *cargs, n, es, et, _lib.method_id(method), _params_ref(params),
                                                  int(sharing), res), "register_graph")
    return _results(res, n)


def register_sequence(clouds, method: str, params: _lib.Params | None = None, device: int = 0,
                      sharing: int = 0, voxel_size: float | None = None, init=None) -> list[PairResult]:
    """register_graph over sequence_edges(len(clouds)): scan i+1 onto scan i (init: the odometry
    prior of every step)."""
    return register_graph(clouds, sequence_edges(len(clouds)), method, params, device, sharing, voxel_size, init)


def register_graph_device(xyz_ptr: int, off, edges, method: str, params: _lib.Params | None = None,
                          device: int = 0, stream: int = 0, sharing: int = 0, init=None) -> list[PairResult]:
    """register_graph for clouds already in HBM: xyz_ptr is the device address of the
    concatenated AoS float64 xyz of every cloud, off the n_clouds+1 point offsets."""
    nc = len(off) - 1
    co = (C.c_int64 * (nc + 1))(*[int(x) for x in off])
    n, es, et = _edge_arrays(edges)
    res, _ = _outputs(n)
    T0 = _init_array(init, n)
    if T0 is not None:
        _registered(_lib.load().se3icp_register_graph_init_device(
            device, nc, C.c_void_p(xyz_ptr), co, n, es, et, T0.ctypes.data_as(_DP), _lib.method_id(method),
            _params_ref(params), int(sharing), res, _stream_arg(stream), None, None), "register_graph_init_device")
        return _results(res, n)
    _registered(_lib.load().se3icp_register_graph_device(device, nc, C.c_void_p(xyz_ptr), co, n, es, et,
                                                         _lib.method_id(method), _params_ref(params), int(sharing),
                                                         res, _stream_arg(stream)), "register_graph_device")
    return _results(res, n)


def register_graph_report(clouds, edges, method: str, params: _lib.Params | None = None, device: int = 0,
                          sharing: int = 0, max_correspondence_distance: float = 0.0, per_point: bool = False,
                          init=None):
    """register_graph plus a PairReport per edge, as register_batch_report: (results, reports)."""
    cl, cargs = _cloud_args(clouds)
    n, es, et = _edge_arrays(edges)
    counts = [cl[int(s)].shape[0] for s, _ in edges]
    res, rep = _outputs(n)
    opts, idx, dist = _per_point_options(max_correspondence_distance, counts, per_point)
    T0 = _init_array(init, n)
    if T0 is not None:
        _registered(_lib.load().se3icp_register_graph_init(device, *cargs, n, es, et, T0.ctypes.data_as(_DP),
                                                           _lib.method_id(method), _params_ref(params), int(sharing),
                                                           res, C.byref(opts), rep), "register_graph_init")
        return _results(res, n), _pair_reports(rep, counts, idx, dist)
    _registered(_lib.load().se3icp_register_graph_report(device, *cargs, n, es, et, _lib.method_id(method),
                                                         _params_ref(params), int(sharing), res, C.byref(opts), rep),
                "register_graph_report")
    return _results(res, n), _pair_reports(rep, counts, idx, dist)


def register_graph_traced(clouds, edges, method: str, params: _lib.Params | None = None, edge: int = 0,
                          max_iters: int = 160, device: int = 0, sharing: int = 0, init=None):
    """register_graph with the per-iteration record of one edge (see register_batch_traced); with
    init the record is the plain run's on the posed source."""
    with _armed_trace(device, edge, _as_xyz(clouds[int(edges[edge][0])]).shape[0], max_iters) as trace:
        res = register_graph(clouds, edges, method, params, device, sharing, init=init)
    return res, trace


# ---- voxel-grid downsample (raw scans -> the clouds the drivers register)
_IP = C.POINTER(C.c_int32)


def voxel_downsample(xyz, voxel_size: float, device: int = 0, return_counts: bool = False):
    """Open3D ``PointCloud::VoxelDownSample`` of one (N, 3) cloud on the GPU
    (se3icp_voxel_downsample): the (M, 3) voxel means, voxels in first-occurrence order.
    return_counts: also the points per voxel and each voxel's lowest input index, (M,) int32."""
    pts = _as_xyz(xyz)
    n = pts.shape[0]
    out = np.empty((max(n, 1), 3))
    cnt = np.empty(max(n, 1), dtype=np.int32)
    fst = np.empty(max(n, 1), dtype=np.int32)
    m = _lib.load().se3icp_voxel_downsample(int(device), pts.ctypes.data_as(_DP), n, float(voxel_size),
                                            out.ctypes.data_as(_DP), cnt.ctypes.data_as(_IP) if return_counts else None,
                                            fst.ctypes.data_as(_IP) if return_counts else None)
    if m < 0:
        raise _lib.Se3IcpError(int(m), "voxel_downsample")
    if return_counts:
        return out[:m].copy(), cnt[:m].copy(), fst[:m].copy()
    return out[:m].copy()


def voxel_downsample_device(xyz_ptr: int, off, voxel_size, out_ptr: int, device: int = 0, stream: int = 0,
                            count_ptr: int = 0, first_ptr: int = 0) -> list[int]:
    """Voxel-downsample clouds resident in HBM into HBM (se3icp_voxel_downsample_device).

    xyz_ptr: device address of the concatenated AoS float64 xyz; off: n_clouds+1 point offsets;
    voxel_size: one value, or one per cloud; out_ptr: device buffer with room for every input
    point.  Returns out_off (n_clouds+1): (out_ptr, out_off) go straight into
    register_batch_device / register_graph_device.  count_ptr / first_ptr: optional int32
    device buffers (points per output voxel, its lowest input index within its cloud)."""
    nc = len(off) - 1
    vs = np.ascontiguousarray(np.broadcast_to(np.asarray(voxel_size, dtype=np.float64), (max(nc, 0),)))
    co = (C.c_int64 * (max(nc, 0) + 1))(*[int(x) for x in off])
    oo = (C.c_int64 * (max(nc, 0) + 1))()
    _lib.check(_lib.load().se3icp_voxel_downsample_device(
        int(device), nc, C.c_void_p(xyz_ptr), co, vs.ctypes.data_as(_DP), C.c_void_p(out_ptr), oo,
        C.c_void_p(count_ptr) if count_ptr else None, C.c_void_p(first_ptr) if first_ptr else None,
        _stream_arg(stream)), "voxel_downsample_device")
    return [int(x) for x in oo]


def _register_graph_voxel(clouds, edges, method, params, device, sharing, voxel_size, init=None):
    """register_graph(voxel_size=...): the raw clouds go to HBM once (torch holds the buffers),
    are downsampled there and registered where they lie."""
    import torch

    cl = [_as_xyz(c) for c in clouds]
    off = np.concatenate([[0], np.cumsum([a.shape[0] for a in cl])]).astype(np.int64)
    if len(cl) == 0 or off[-1] == 0:
        raise _lib.Se3IcpError(_lib.ERR_EMPTY_CLOUD, "register_graph(voxel_size=...)")
    dev = torch.device("cuda", int(device) & 0xff)
    raw = torch.from_numpy(np.concatenate(cl)).to(dev)
    down = torch.empty_like(raw)
    torch.cuda.synchronize(dev)  # the engine's stream is not torch's
    out_off = voxel_downsample_device(raw.data_ptr(), off, voxel_size, down.data_ptr(), device=device)
    return register_graph_device(down.data_ptr(), out_off, edges, method, params, device=device, sharing=sharing,
                                 init=init)


def last_graph_stats(device: int = 0) -> dict:
    """Counters of the last register_graph on `device`, or of its last device batch that looked
    for shared clouds (se3icp_last_graph_stats, se3icp_set_batch_sharing)."""
    out = (C.c_int64 * len(_lib.GRAPH_STATS))()
    _lib.check(_lib.load().se3icp_last_graph_stats(device, out, len(_lib.GRAPH_STATS)), "last_graph_stats")
    return {k: int(out[i]) for i, k in enumerate(_lib.GRAPH_STATS)}


def set_batch_sharing(level: int, device: int = 0) -> None:
    """What the device batch entries (register_batch_device, register_batch_report_device,
    DeviceBatchRunner) do about cloud slots that hold the same cloud, detected by content on the
    device (se3icp_set_batch_sharing): 0 the highest level built (the default), 1 nothing (the
    plain batch), 2 one neighbour selection per (cloud, normalization) class.  Results are
    bitwise the same at every level; last_graph_stats() describes the last such call."""
    _lib.check(_lib.load().se3icp_set_batch_sharing(int(device), int(level)), "set_batch_sharing")


def toldi_frames(pts, k: int, device: int = 0) -> np.ndarray:
    """computeAllTOLDISE3FramesOMP (ISR.cpp:318-331): (N, 4, 4) frames."""
    pts = _as_xyz(pts)
    out = np.zeros((pts.shape[0], 4, 4))
    _lib.check(_lib.load().se3icp_toldi_frames(device, pts.ctypes.data_as(C.POINTER(C.c_double)), pts.shape[0], k,
                                               out.ctypes.data_as(C.POINTER(C.c_double))), "toldi_frames")
    return out


def knn_self(pts, k: int, device: int = 0) -> np.ndarray:
    """KDTreeFlann::SearchKNN of every point in its own cloud: (N, k) indices."""
    pts = _as_xyz(pts)
    out = np.zeros((pts.shape[0], k), np.int32)
    _lib.check(_lib.load().se3icp_knn_self(device, pts.ctypes.data_as(C.POINTER(C.c_double)), pts.shape[0], k,
                                           out.ctypes.data_as(C.POINTER(C.c_int32))), "knn_self")
    return out


def estimate_normals(pts, k: int = 30, device: int = 0) -> np.ndarray:
    """PointCloud::EstimateNormals(KDTreeSearchParamKNN(k)) (ISR.cpp:643)."""
    pts = _as_xyz(pts)
    out = np.zeros_like(pts)
    _lib.check(_lib.load().se3icp_estimate_normals(device, pts.ctypes.data_as(C.POINTER(C.c_double)), pts.shape[0],
                                                   k, out.ctypes.data_as(C.POINTER(C.c_double))), "estimate_normals")
    return out


def nearest_neighbors(query, data, device: int = 0):
    """Exact 1-NN in 3 or 12 dims (ISR.cpp:402-416 / 444-470); returns (idx, d2, n_rechecked)."""
    q = np.ascontiguousarray(query, dtype=np.float64)
    d = np.ascontiguousarray(data, dtype=np.float64)
    dim = d.shape[1]
    idx = np.zeros(q.shape[0], np.int32)
    d2 = np.zeros(q.shape[0])
    nr = C.c_int32(0)
    dp = C.POINTER(C.c_double)
    _lib.check(_lib.load().se3icp_nn(device, q.ctypes.data_as(dp), q.shape[0], d.ctypes.data_as(dp), d.shape[0], dim,
                                     idx.ctypes.data_as(C.POINTER(C.c_int32)), d2.ctypes.data_as(dp), C.byref(nr)),
               "nn")
    return idx, d2, int(nr.value)


def nearest_neighbors_sequence(query, data, poses, alpha: float = 1.0, restart_at: int = 0, device: int = 0) -> dict:
    """The loop's NN stage over a given pose sequence (se3icp_nn_sequence): step k (1-based) is
    iteration k of a one-pair run whose pose is poses[k - 1] ((n_steps, 4, 4) or (n_steps, 16),
    row-major).  query (nq, dim), data (nd, dim), dim 3 or 12; a 12-D query row is
    [alpha x, alpha y, alpha z, t] with (x y z) orthonormal (not checked).  Returns per step and
    query (n_steps, nq) `idx`, `dist` (f32), `cert_d1`, `cert_l2` (f32), `cert_iter`, `cert_j`, and
    per step `searched`, `single`, `rechecked`."""
    q = np.ascontiguousarray(query, dtype=np.float64)
    d = np.ascontiguousarray(data, dtype=np.float64)
    T = np.ascontiguousarray(poses, dtype=np.float64)
    if q.ndim != 2 or d.ndim != 2 or q.shape[1] != d.shape[1] or T.size % 16 or T.ndim < 2:
        raise _lib.Se3IcpError(_lib.ERR_INVALID_ARG, "nn_sequence: shapes")
    ns, nq = T.size // 16, q.shape[0]
    out = {k: np.zeros((ns, nq), t) for k, t in (("idx", np.int32), ("dist", np.float32), ("cert_d1", np.float32),
                                                 ("cert_l2", np.float32), ("cert_iter", np.int32),
                                                 ("cert_j", np.int32))}
    out.update({k: np.zeros(ns, np.int32) for k in ("searched", "single", "rechecked")})
    dp, ip, fp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    ptr = lambda k: out[k].ctypes.data_as(fp if out[k].dtype == np.float32 else ip)
    _lib.check(_lib.load().se3icp_nn_sequence(
        int(device), q.ctypes.data_as(dp), nq, d.ctypes.data_as(dp), d.shape[0], int(d.shape[1]), float(alpha), ns,
        T.ctypes.data_as(dp), int(restart_at), ptr("idx"), ptr("dist"), ptr("cert_d1"), ptr("cert_l2"),
        ptr("cert_iter"), ptr("cert_j"), ptr("searched"), ptr("single"), ptr("rechecked")), "nn_sequence")
    return out


def set_lrf_seeding(mode: int, device: int = 0) -> None:
    """How the classes of one cloud seed each other's neighbour selection on the engine behind
    `device` (se3icp_set_lrf_seeding): 0 a cloud's later classes start from its first class's
    neighbour distances (the default), 1 off, 2 / 3 diagnostics (every seed halved: the
    certificate fails; every seed times 4: loose seeds).  Results are bitwise the same in every
    mode; last_seed_stats() describes the last call."""
    _lib.check(_lib.load().se3icp_set_lrf_seeding(int(device), int(mode)), "set_lrf_seeding")


def last_seed_stats(device: int = 0) -> dict:
    """Seeding counters of the last registration call on `device` (se3icp_last_seed_stats)."""
    out = (C.c_int64 * len(_lib.SEED_STATS))()
    _lib.check(_lib.load().se3icp_last_seed_stats(int(device), out, len(_lib.SEED_STATS)), "last_seed_stats")
    return {k: int(out[i]) for i, k in enumerate(_lib.SEED_STATS)}


def set_lrf_taking(mode: int, device: int = 0) -> None:
    """Whether a seeded class that has its source's kd-tree order takes the source's neighbour
    lists, re-checked under its own scale, instead of searching, on the engine behind `device`
    (se3icp_set_lrf_taking): 0 take (the default), 1 off, 2 a diagnostic (every stored bound
    halved: every wavefront is redone as a seeded one).  Results are bitwise the same in every
    mode; last_take_stats() describes the last call."""
    _lib.check(_lib.load().se3icp_set_lrf_taking(int(device), int(mode)), "set_lrf_taking")


def last_take_stats(device: int = 0) -> dict:
    """Taking counters of the last registration call on `device` (se3icp_last_take_stats)."""
    out = (C.c_int64 * len(_lib.TAKE_STATS))()
    _lib.check(_lib.load().se3icp_last_take_stats(int(device), out, len(_lib.TAKE_STATS)), "last_take_stats")
    return {k: int(out[i]) for i, k in enumerate(_lib.TAKE_STATS)}


def set_tree_sharing(mode: int, device: int = 0) -> None:
    """Whether the later slots of a confirmed cloud take its first slot's kd-tree order on the
    engine behind `device` (se3icp_set_tree_sharing): 0 adopt (the default), 1 off, every slot
    builds its own trees.  Results are bitwise the same; last_tree_stats() describes the last
    call."""
    _lib.check(_lib.load().se3icp_set_tree_sharing(int(device), int(mode)), "set_tree_sharing")


def last_tree_stats(device: int = 0) -> dict:
    """Trees built and adopted by the last registration call on `device` (se3icp_last_tree_stats)."""
    out = (C.c_int64 * len(_lib.TREE_STATS))()
    _lib.check(_lib.load().se3icp_last_tree_stats(int(device), out, len(_lib.TREE_STATS)), "last_tree_stats")
    return {k: int(out[i]) for i, k in enumerate(_lib.TREE_STATS)}


def set_lrf_exact(mode, device: int = 0) -> None:
    """Diagnostic: which kernels compute the setup's kNN / TOLDI / normals.  0 / False: the
    default (k_lrf8 + hand-overs); 1 / True: the exact one-query-per-wavefront kernel for every
    point; 2: the global-buffer kernel (any k) for every point.  All bitwise equal."""
    _lib.check(_lib.load().se3icp_set_lrf_exact(device, int(mode)))


def set_nn_events(on: bool, device: int = 0) -> None:
    """HIP events around the SE(3) NN grids of timed batches (default on; they fill
    time_se3_correspondence_search_ms, and each leaves the GPU idle a few microseconds)."""
    _lib.check(_lib.load().se3icp_set_nn_events(device, 1 if on else 0))


def set_profiling(on: bool, device: int = 0) -> None:
    """HIP events around every loop stage (not only the NN grids) from the next batch on."""
    _lib.check(_lib.load().se3icp_set_profiling(device, 1 if on else 0))


def last_kernel_times(device: int = 0) -> dict:
    keys = DeviceBatchRunner._KT_KEYS
    out = (C.c_double * len(keys))()
    _lib.check(_lib.load().se3icp_last_kernel_times_n(device, out, len(keys)))
    return dict(zip(keys, list(out)))
