"""include/m3s_gn.h: the reference's three Gauss-Newton entry points, their
stepwise (sharded) form, the diagnostics and knobs, and the tracker."""
import ctypes

import torch

from ._abi import (_F32, _I32, _I64, _INT, _P, _SIZE, _VP, _call, _caller_workspace, _check, _layout, _p, _raise,
                   _same_device, _stream, _sym, _workspace)

MODE_POINTS, MODE_RAYS, MODE_CALIB = 0, 1, 2
INFO_ITERS, INFO_SOLVE_FAIL, INFO_BAD_EDGE, INFO_CONVERGED, INFO_N_UNIQUE = 0, 1, 2, 3, 4
EDGE_SUM_STRIDE = 36


class GnArgs(ctypes.Structure):
    """Mirror of ``m3s_gn_args`` (include/m3s_gn.h)."""

    _fields_ = [
        ("Twc", _VP), ("Xs", _VP), ("Cs", _VP), ("ii", _VP), ("jj", _VP), ("idx_ii2jj", _VP), ("valid_match", _VP),
        ("Q", _VP), ("K", _VP), ("N", _I64), ("HW", _I64), ("E", _I64), ("mode", _INT), ("sigma_a", _F32),
        ("sigma_b", _F32), ("C_thresh", _F32), ("Q_thresh", _F32), ("height", _INT), ("width", _INT),
        ("pixel_border", _INT), ("z_eps", _F32), ("max_iter", _INT), ("delta_thresh", _F32), ("dx_out", _VP),
        ("info", _VP), ("workspace", _VP), ("workspace_bytes", _SIZE), ("idx_i32", _INT),
    ]


class TrackArgs(ctypes.Structure):
    """Mirror of ``m3s_track_args`` (include/m3s_gn.h)."""

    _fields_ = [
        ("Xf", _VP), ("Xk", _VP), ("Qk", _VP), ("valid", _VP), ("T_WCf", _VP), ("T_WCk", _VP), ("K", _VP), ("HW", _I64),
        ("height", _INT), ("width", _INT), ("pixel_border", _INT), ("z_eps", _F32), ("sigma_a", _F32),
        ("sigma_b", _F32), ("huber_k", _F32), ("max_iters", _INT), ("rel_error", _F32), ("delta_norm", _F32),
        ("sync_every", _INT), ("T_WCf_out", _VP), ("T_CkCf_out", _VP), ("info", _VP), ("workspace", _VP),
        ("workspace_bytes", _SIZE),
    ]


class TrackFrameArgs(ctypes.Structure):
    """Mirror of ``m3s_track_frame_args`` (include/m3s_gn.h)."""

    _fields_ = [
        ("Xf_canon", _VP), ("Cf_sum", _VP), ("Xk_canon", _VP), ("Ck_sum", _VP), ("idx_f2k", _VP), ("valid_match", _VP),
        ("Qk", _VP), ("T_WCf", _VP), ("T_WCk", _VP), ("K", _VP), ("HW", _I64), ("Nf", _I32), ("Nk", _I32),
        ("height", _INT), ("width", _INT), ("C_conf", _F32), ("Q_conf", _F32), ("pixel_border", _INT), ("z_eps", _F32),
        ("sigma_a", _F32), ("sigma_b", _F32), ("huber_k", _F32), ("max_iters", _INT), ("rel_error", _F32),
        ("delta_norm", _F32), ("sync_every", _INT), ("T_WCf_out", _VP), ("T_CkCf_out", _VP), ("info", _VP),
        ("stats", _VP), ("Xf_out", _VP), ("Xk_out", _VP), ("valid_opt_out", _VP), ("workspace", _VP),
        ("workspace_bytes", _SIZE),
    ]


STAT_N_OPT, STAT_N_KF, STAT_N_UNIQUE = 0, 1, 2

_GN = (_INT, [_P(GnArgs), _VP])
# symbol -> (restype, argtypes): include/m3s_gn.h
_SIGNATURES = {
    "m3s_gn_workspace_size": (_SIZE, [_I64] * 3),
    "m3s_gauss_newton_points": _GN,
    "m3s_gauss_newton_rays": _GN,
    "m3s_gauss_newton_calib": _GN,
    "m3s_gn_prepare": _GN,
    "m3s_gn_linearize": (_INT, [_P(GnArgs), _I64, _I64, _VP, _VP]),
    "m3s_gn_solve": (_INT, [_P(GnArgs), _VP, _VP]),
    "m3s_gn_release": _GN,
    "m3s_track_workspace_size": (_SIZE, [_I64]),
    "m3s_track_rays_sim3": (_INT, [_P(TrackArgs), _VP]),
    "m3s_track_calib_sim3": (_INT, [_P(TrackArgs), _VP]),
    "m3s_track_frame_workspace_size": (_SIZE, [_I64]),
    "m3s_track_frame": (_INT, [_P(TrackFrameArgs), _VP]),
    "m3s_version": (ctypes.c_char_p, []),
    "m3s_sparse_plan_debug": (_I64, [_I32, _I64, _VP, _VP, _I32, _I32, _VP, _I64, _VP]),
    "m3s_gn_layout_debug": (_SIZE, [_I64, _I64, _I64, _VP]),
    "m3s_gn_plan_path_debug": (ctypes.c_char_p, [_I64, _I64, _I64, _VP, _VP]),
    "m3s_debug_stamps": (_INT, [_INT, _VP]),
    "m3s_debug_sim3": (_INT, [_INT, _VP, _VP, _VP, _I64, _VP]),
    "m3s_debug_copy": (_INT, [_VP, _VP, _I64, _INT, _VP]),
    "m3s_set_knob": (_INT, [ctypes.c_char_p, _INT]),
    "m3s_debug_call_timing": (_INT, [_INT]),
    "m3s_debug_call_times": (_INT, [_VP, _VP, _INT]),
}


def version() -> str:
    return _sym("m3s_version")().decode()


# the rows of M3S_PLAN_SECTIONS (csrc/m3s_symbolic.h), in order (tests/test_sparse_plan.py)
PLAN_SECTIONS = ("perm", "col_ptr", "col_row", "col_slot", "lev_ptr", "lev_col", "dtr_ptr",
                 "dtr_slot", "dtr_p", "task_lev_ptr", "task_dst", "task_col", "task_tr_ptr", "tr_a",
                 "tr_b", "asm_ptr", "asm_edge", "g_ptr", "g_edge", "ctask_ptr", "items", "wave_ptr", "witems",
                 "part_q0", "part_q1", "part_tgt", "dpart_ptr", "opart_ptr", "clq", "corder", "ctask0")

LAYOUT_SECTIONS = ("flags", "rank_i", "rank_j", "first", "partials", "edge_sums", "A", "fin",
                   "plan", "Lblk", "Dinv", "tail", "eorder", "planes", "total")

SIM3_OPS = {"exp": (0, 7, None, 8), "retract": (1, 7, 8, 8), "compose": (2, 8, 8, 8), "inverse": (3, 8, None, 8),
            "relative": (4, 8, 8, 8), "act": (5, 8, 3, 3), "act_matrix": (6, 8, 3, 3), "adjT_inv": (7, 8, None, 49),
            "retract_f32": (8, 7, 8, 8)}


def debug_sim3(op: str, a: torch.Tensor, b: torch.Tensor = None) -> torch.Tensor:
    """The device Sim(3) helpers of the hot path on [n, ...] float32 device
    tensors (m3s_debug_sim3; diagnostics/tests). op in SIM3_OPS."""
    code, wa, wb, wo = SIM3_OPS[op]
    a = a.contiguous()
    _check(a, "a", torch.float32)
    n = a.numel() // wa
    if a.numel() != n * wa:
        raise RuntimeError(f"debug_sim3({op}): a must be [n, {wa}]")
    if wb is not None:
        if b is None:
            raise RuntimeError(f"debug_sim3({op}) needs b")
        b = b.contiguous()
        _check(b, "b", torch.float32)
        if b.numel() != n * wb:
            raise RuntimeError(f"debug_sim3({op}): b must be [n, {wb}]")
    out = torch.empty(n, wo, dtype=torch.float32, device=a.device)
    _call("m3s_debug_sim3", code, _p(a), _p(b), _p(out), n, _stream(a.device))
    return out


def set_knob(name: str, value: int) -> int:
    """Set a solver knob for the calls that follow (include/m3s_gn.h
    m3s_set_knob); returns the previous value."""
    old = _sym("m3s_set_knob")(name.encode(), int(value))
    if old == -(1 << 30):
        raise RuntimeError(f"unknown knob {name!r}")
    return old


class knob:
    """``with knob("df", 0): ...`` — a knob set for the block, restored after."""

    def __init__(self, name: str, value: int):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = set_knob(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_knob(self.name, self.old)


def debug_call_timing(enable: bool) -> None:
    """Turn in-call launch timing on or off (m3s_debug_call_timing); the
    record of the calls that follow is read by debug_call_times()."""
    _call("m3s_debug_call_timing", 1 if enable else 0)


def debug_call_times(cap: int = 4096):
    """[(kind, ms)] of the timed calls since debug_call_timing(True), in launch
    order; kind 0 = first-iteration (gathering) linearize, 1 = packed
    linearize, 2 = solve launches of one iteration."""
    import numpy as np

    ms = np.zeros(cap, np.float32)
    kinds = np.zeros(cap, np.int32)
    n = _sym("m3s_debug_call_times")(ms.ctypes.data, kinds.ctypes.data, cap)
    if n < 0:
        _raise(n, "m3s_debug_call_times")
    n = min(n, cap)
    return [(int(kinds[k]), float(ms[k])) for k in range(n)]


def debug_copy(src: torch.Tensor, dst: torch.Tensor, blocks: int = 4096):
    """dst <- src by the 16-B streaming copy kernel (m3s_debug_copy)."""
    _check(src, "src")
    _check(dst, "dst")
    nb = src.numel() * src.element_size()
    if dst.numel() * dst.element_size() < nb:
        raise RuntimeError("debug_copy: dst too small")
    _call("m3s_debug_copy", _p(src), _p(dst), nb, int(blocks), _stream(src.device))


def workspace_layout(N, HW, E):
    """Byte offsets of the GN workspace sections (diagnostics/tests)."""
    return _layout("m3s_gn_layout_debug", LAYOUT_SECTIONS, N, HW, E)


def plan_path(N, HW, ri, rj) -> str:
    """The launch path the solver takes for N poses, HW pixels and the edge
    ranks (ri, rj) under the current knobs (m3s_gn_plan_path_debug; CPU only):
    "dense", "lds_plan", "lds", "chip", "global_split" or "global"."""
    import numpy as np

    ri = np.ascontiguousarray(ri, dtype=np.int32)
    rj = np.ascontiguousarray(rj, dtype=np.int32)
    name = None
    if ri.size == rj.size:
        name = _sym("m3s_gn_plan_path_debug")(int(N), int(HW), ri.size, _VP(ri.ctypes.data), _VP(rj.ctypes.data))
    if name is None:
        raise RuntimeError("plan_path: bad arguments")
    return name.decode()


def sparse_plan(N, ri, rj, split=0, max_parts=0):
    """Host symbolic plan of the block-sparse LLT (diagnostics/tests; CPU only).
    split > 0: long update lists cut into PART items (global-factor solves).
    The dense tail (clq) follows M3S_DENSE_TAIL_MIN like the solver."""
    import numpy as np

    ri = np.ascontiguousarray(ri, dtype=np.int32)
    rj = np.ascontiguousarray(rj, dtype=np.int32)
    meta = np.zeros(4 + len(PLAN_SECTIONS), np.int32)
    args = (int(N), ri.size, _VP(ri.ctypes.data), _VP(rj.ctypes.data), int(split), int(max_parts))
    plan_debug = _sym("m3s_sparse_plan_debug")
    n = plan_debug(*args, None, 0, _VP(meta.ctypes.data))
    out = np.zeros(max(n, 1), np.int32)
    plan_debug(*args, _VP(out.ctypes.data), n, _VP(meta.ctypes.data))
    offs = list(meta[3:3 + len(PLAN_SECTIONS)]) + [n]
    plan = {"m": int(meta[0]), "S": int(meta[1]), "levels": int(meta[2]),
            "n_parts": int(meta[3 + len(PLAN_SECTIONS)])}
    for k, name in enumerate(PLAN_SECTIONS):
        plan[name] = out[offs[k]:]
    m, S, L, NP = plan["m"], plan["S"], plan["levels"], plan["n_parts"]
    T = int(plan["task_lev_ptr"][L])
    sp = NP > 0 or split > 0
    nc = int(plan["clq"][0])  # dense-tail columns: not dataflow items
    plan["nc"] = nc
    n_items = (m - nc) + (T - nc * (nc - 1) // 2) + NP
    lens = {"perm": m, "col_ptr": m + 1, "lev_ptr": L + 1, "lev_col": m, "dtr_ptr": m + 1,
            "task_lev_ptr": L + 1, "task_dst": T, "task_col": T, "task_tr_ptr": T + 1,
            "asm_ptr": S + 1, "g_ptr": m + 1, "ctask_ptr": m + 1, "clq": 2 + nc + nc * nc,
            "items": n_items, "wave_ptr": 2, "witems": n_items,
            "part_q0": NP, "part_q1": NP, "part_tgt": NP,
            "dpart_ptr": m + 1 if sp else 0, "opart_ptr": T + 1 if sp else 0,
            "corder": m - nc, "ctask0": m}
    for name, ln in lens.items():
        plan[name] = plan[name][:ln]
    nnz = int(plan["col_ptr"][m])
    plan["col_row"], plan["col_slot"] = plan["col_row"][:nnz], plan["col_slot"][:nnz]
    nd = int(plan["dtr_ptr"][m])
    plan["dtr_slot"], plan["dtr_p"] = plan["dtr_slot"][:nd], plan["dtr_p"][:nd]
    nt = int(plan["task_tr_ptr"][T])
    plan["tr_a"], plan["tr_b"] = plan["tr_a"][:nt], plan["tr_b"][:nt]
    plan["asm_edge"] = plan["asm_edge"][:int(plan["asm_ptr"][S])]
    plan["g_edge"] = plan["g_edge"][:int(plan["g_ptr"][m])]
    return plan


def make_gn_args(mode, Twc, Xs, Cs, ii, jj, idx_ii2jj, valid_match, Q, K=None, *, dx=None, info=None,
                 workspace=None, **scalars):
    """Validate reference-layout tensors and fill an ``m3s_gn_args`` (scalars: fill_gn_args' keywords).
    Returns (args, keepalive) — keepalive holds every tensor the struct points to."""
    for name, t in (("Twc", Twc), ("Xs", Xs), ("Cs", Cs)) + ((("K", K),) if K is not None else ()):
        _check(t, name, torch.float32)
    _check(ii, "ii", torch.int64)
    _check(jj, "jj", torch.int64)
    # int64 as the reference passes it; int32 from the device edge store
    _check(idx_ii2jj, "idx_ii2jj", (torch.int64, torch.int32))
    _check(valid_match, "valid_match", torch.bool)
    _check(Q, "Q", torch.float32)
    N, HW = int(Xs.shape[0]), int(Xs.shape[1])
    E = int(ii.shape[0])
    if Xs.dim() != 3 or Xs.shape[2] != 3:
        raise RuntimeError("Xs must be [N, HW, 3]")
    if Twc.numel() != 8 * N:
        raise RuntimeError(f"Twc must be [N, 8] with N = Xs.size(0) = {N}")
    if Cs.numel() != N * HW:
        raise RuntimeError("Cs must be [N, HW, 1]")
    if jj.numel() != E or idx_ii2jj.numel() != E * HW or valid_match.numel() != E * HW or Q.numel() != E * HW:
        raise RuntimeError("edge tensors must be [E, HW(,1)] with E = ii.size(0)")
    dev = Xs.device
    # no fill launches: m3s_gn_prepare zeroes dx and uploads info on the stream
    if dx is None:
        dx = torch.empty(max(N - 1, 0), 7, dtype=torch.float32, device=dev)
    if info is None:
        info = torch.empty(8, dtype=torch.int32, device=dev)
    ws_bytes = int(_sym("m3s_gn_workspace_size")(N, HW, E))
    if workspace is None or workspace.numel() < ws_bytes:
        workspace = _workspace(ws_bytes, dev)
    return fill_gn_args(mode, Twc, Xs, Cs, ii, jj, idx_ii2jj, valid_match, Q, K, N, HW, E, dx=dx, info=info,
                        workspace=workspace, **scalars)


def fill_gn_args(mode, Twc, Xs, Cs, ii, jj, idx_ii2jj, valid_match, Q, K, N, HW, E, *, dx, info, workspace,
                 sigma_a=0.0, sigma_b=0.0, C_thresh=0.0, Q_thresh=0.0, height=0, width=0, pixel_border=0,
                 z_eps=0.0, max_iter=0, delta_thresh=0.0):
    """An ``m3s_gn_args`` over tensors its caller has checked; E is given, not read from the edge tensors
    (the stepwise API takes a slice of the edges under the full id lists). Returns (args, keepalive)."""
    a = GnArgs()
    a.Twc, a.Xs, a.Cs, a.ii, a.jj = _p(Twc), _p(Xs), _p(Cs), _p(ii), _p(jj)
    a.idx_ii2jj, a.valid_match, a.Q, a.K = _p(idx_ii2jj), _p(valid_match), _p(Q), _p(K)
    a.idx_i32 = 1 if idx_ii2jj.dtype == torch.int32 else 0
    a.N, a.HW, a.E, a.mode = int(N), int(HW), int(E), mode
    a.sigma_a, a.sigma_b = float(sigma_a), float(sigma_b)
    a.C_thresh, a.Q_thresh = float(C_thresh), float(Q_thresh)
    a.height, a.width, a.pixel_border = int(height), int(width), int(pixel_border)
    a.z_eps = float(z_eps)
    a.max_iter, a.delta_thresh = int(max_iter), float(delta_thresh)
    a.dx_out, a.info = _p(dx), _p(info)
    a.workspace, a.workspace_bytes = _p(workspace), workspace.numel()
    keep = dict(Twc=Twc, Xs=Xs, Cs=Cs, ii=ii, jj=jj, idx=idx_ii2jj, valid=valid_match, Q=Q, K=K,
                dx=dx, info=info, workspace=workspace)
    return a, keep


def _run_gn(fn_name, a, keep):
    st = _stream(keep["Xs"].device)
    rc = _sym(fn_name)(ctypes.byref(a), st)
    # the per-call workspace goes back to the caching allocator: drop its host
    # state too (m3s_gn_release: no stream sync; the call returns as soon as
    # its launches are queued)
    rc_rel = _sym("m3s_gn_release")(ctypes.byref(a), st)
    _raise(rc, fn_name)
    _raise(rc_rel, "m3s_gn_release")
    return [keep["dx"]]


# ------------------------------------------------- reference entry points --
def gauss_newton_points(Twc, Xs, Cs, ii, jj, idx_ii2jj, valid_match, Q, sigma_point, C_thresh,
                        Q_thresh, max_iter, delta_thresh, *, info=None):
    """gn.cpp:3-27 / gn_kernels.cu:725-811."""
    a, keep = make_gn_args(MODE_POINTS, Twc, Xs, Cs, ii, jj, idx_ii2jj, valid_match, Q,
                           sigma_a=sigma_point, C_thresh=C_thresh, Q_thresh=Q_thresh,
                           max_iter=max_iter, delta_thresh=delta_thresh, info=info)
    return _run_gn("m3s_gauss_newton_points", a, keep)


def gauss_newton_rays(Twc, Xs, Cs, ii, jj, idx_ii2jj, valid_match, Q, sigma_ray, sigma_dist,
                      C_thresh, Q_thresh, max_iter, delta_thresh, *, info=None):
    """gn.cpp:29-54 / gn_kernels.cu:1140-1228."""
    a, keep = make_gn_args(MODE_RAYS, Twc, Xs, Cs, ii, jj, idx_ii2jj, valid_match, Q,
                           sigma_a=sigma_ray, sigma_b=sigma_dist, C_thresh=C_thresh,
                           Q_thresh=Q_thresh, max_iter=max_iter, delta_thresh=delta_thresh,
                           info=info)
    return _run_gn("m3s_gauss_newton_rays", a, keep)


def gauss_newton_calib(Twc, Xs, Cs, K, ii, jj, idx_ii2jj, valid_match, Q, height, width,
                       pixel_border, z_eps, sigma_pixel, sigma_depth, C_thresh, Q_thresh, max_iter,
                       delta_thresh, *, info=None):
    """gn.cpp:56-85 / gn_kernels.cu:1546-1638."""
    a, keep = make_gn_args(MODE_CALIB, Twc, Xs, Cs, ii, jj, idx_ii2jj, valid_match, Q, K,
                           sigma_a=sigma_pixel, sigma_b=sigma_depth, C_thresh=C_thresh,
                           Q_thresh=Q_thresh, height=height, width=width,
                           pixel_border=pixel_border, z_eps=z_eps, max_iter=max_iter,
                           delta_thresh=delta_thresh, info=info)
    return _run_gn("m3s_gauss_newton_calib", a, keep)


# -------------------------------------------------- stepwise (sharded) ---
def gn_prepare(a, keep):
    _call("m3s_gn_prepare", ctypes.byref(a), _stream(keep["Xs"].device))


def gn_linearize(a, keep, edge_begin, edge_end, edge_sums):
    """edge_sums None: the linearize launches alone (a timing hook)."""
    if edge_sums is not None:
        _check(edge_sums, "edge_sums", torch.float64)
    _call("m3s_gn_linearize", ctypes.byref(a), int(edge_begin), int(edge_end), _p(edge_sums),
          _stream(keep["Xs"].device))


def gn_release(a, keep):
    _call("m3s_gn_release", ctypes.byref(a), _stream(keep["Xs"].device))


def gn_solve(a, keep, edge_sums):
    _check(edge_sums, "edge_sums", torch.float64)
    _call("m3s_gn_solve", ctypes.byref(a), _p(edge_sums), _stream(keep["Xs"].device))


# ------------------------------------------------------------ tracker ---
def _poses(T_WCf, T_WCk, K):
    """The two poses made contiguous and checked, and K when there is one."""
    T_WCf, T_WCk = T_WCf.contiguous(), T_WCk.contiguous()
    _check(T_WCf, "T_WCf", torch.float32)
    _check(T_WCk, "T_WCk", torch.float32)
    if K is not None:
        _check(K, "K", torch.float32)
    return T_WCf, T_WCk


def _track(fn, Xf, Xk, T_WCf, T_WCk, Qk, valid, K, img_size, sigma_a, sigma_b, huber_k,
           max_iters, rel_error, delta_norm, pixel_border=0, z_eps=0.0, sync_every=5, workspace=None):
    for name, t in (("Xf", Xf), ("Xk", Xk), ("Qk", Qk)):
        _check(t, name, torch.float32)
    _check(valid, "valid", torch.bool)
    T_WCf, T_WCk = _poses(T_WCf, T_WCk, K)
    HW = int(Xk.shape[0])
    if Xf.numel() != 3 * HW or Xk.numel() != 3 * HW or Qk.numel() != HW or valid.numel() != HW:
        raise RuntimeError("tracker inputs must be Xf/Xk [HW,3], Qk/valid [HW,1]")
    dev = Xk.device
    out_f = torch.empty(1, 8, dtype=torch.float32, device=dev)
    out_r = torch.empty(1, 8, dtype=torch.float32, device=dev)
    info = torch.zeros(8, dtype=torch.int32, device=dev)
    ws = _caller_workspace(workspace, track_workspace_size(HW), dev, "tracker")
    a = TrackArgs()
    a.Xf, a.Xk, a.Qk, a.valid = _p(Xf), _p(Xk), _p(Qk), _p(valid)
    a.T_WCf, a.T_WCk, a.K = _p(T_WCf), _p(T_WCk), _p(K)
    a.HW = HW
    h, w = (int(img_size[0]), int(img_size[1])) if img_size is not None else (0, 0)
    a.height, a.width, a.pixel_border, a.z_eps = h, w, int(pixel_border), float(z_eps)
    a.sigma_a, a.sigma_b, a.huber_k = float(sigma_a), float(sigma_b), float(huber_k)
    a.max_iters, a.rel_error, a.delta_norm = int(max_iters), float(rel_error), float(delta_norm)
    a.sync_every = int(sync_every)
    a.T_WCf_out, a.T_CkCf_out, a.info = _p(out_f), _p(out_r), _p(info)
    a.workspace, a.workspace_bytes = _p(ws), ws.numel()
    _call(fn, ctypes.byref(a), _stream(dev))
    del ws  # stream-ordered by the caching allocator
    return out_f, out_r, info


def track_workspace_size(HW):
    """Bytes of the tracker workspace for an image of HW pixels."""
    return int(_sym("m3s_track_workspace_size")(int(HW)))


def track_rays_sim3(Xf, Xk, T_WCf, T_WCk, Qk, valid, sigma_ray, sigma_dist, huber_k, max_iters,
                    rel_error, delta_norm, sync_every=5, workspace=None):
    """Device form of FrameTracker.opt_pose_ray_dist_sim3 (tracker.py:173-214).
    Returns (T_WCf [1,8], T_CkCf [1,8], info int32[8]); info[1] != 0 means the
    Cholesky failed (the reference raises; tracker.py:91-93)."""
    return _track("m3s_track_rays_sim3", Xf, Xk, T_WCf, T_WCk, Qk, valid, None, None, sigma_ray,
                  sigma_dist, huber_k, max_iters, rel_error, delta_norm, sync_every=sync_every,
                  workspace=workspace)


def track_calib_sim3(Xf, Xk, T_WCf, T_WCk, Qk, valid, K, img_size, sigma_pixel, sigma_depth,
                     huber_k, max_iters, rel_error, delta_norm, pixel_border, z_eps, sync_every=5,
                     workspace=None):
    """Device form of FrameTracker.opt_pose_calib_sim3 (tracker.py:216-266);
    Xf/Xk already constrained to rays, meas_k formed on device."""
    return _track("m3s_track_calib_sim3", Xf, Xk, T_WCf, T_WCk, Qk, valid, K, img_size,
                  sigma_pixel, sigma_depth, huber_k, max_iters, rel_error, delta_norm,
                  pixel_border=pixel_border, z_eps=z_eps, sync_every=sync_every, workspace=workspace)


def track_frame_workspace_size(HW):
    """Bytes of the track_frame workspace for an image of HW pixels."""
    return int(_sym("m3s_track_frame_workspace_size")(int(HW)))


def track_frame(Xf_canon, Cf_sum, Nf, Xk_canon, Ck_sum, Nk, idx_f2k, valid_match, Qk, T_WCf, T_WCk,
                K, img_size, C_conf, Q_conf, sigma_a, sigma_b, huber_k, max_iters, rel_error,
                delta_norm, pixel_border=0, z_eps=0.0, sync_every=0, workspace=None,
                return_prepared=False, out=None):
    """FrameTracker.track from the matches to the refined pose on the device
    (new entry point; m3s_track_frame): get_points_poses (tracker.py:129-154),
    valid_opt / valid_kf (:60-65) and the three counts behind match_frac,
    match_frac_k and unique_frac_f (:67, :104-108) in three launches, then the
    launches of track_rays_sim3 (K is None) or track_calib_sim3 on the result.

    Xf_canon, Xk_canon [HW,3] f32; Cf_sum, Ck_sum [HW(,1)] f32, the summed
    confidences (Pointmap.C) with their update counts Nf, Nk (Pointmap.N);
    idx_f2k [HW] (or [1,HW]) int32 as match_dense writes it, every entry in
    [0, HW) -- not scanned; valid_match [HW(,1)] bool; Qk [HW(,1)] f32; T_WCf,
    T_WCk [8] or [1,8]; K [3,3] f32 or None (rays mode); img_size (H, W) with
    H * W == HW; sigma_a / sigma_b as track_rays_sim3 (rays) or
    track_calib_sim3 (calib) name them.

    -> (T_WCf [1,8], T_CkCf [1,8], info int32[8], stats int32[4]) with stats =
    (n_opt, n_kf, n_unique, 0); with return_prepared=True also (Xf_g [HW,3],
    Xk_g [HW,3], valid_opt [HW,1] bool), the rows the tracker launches read.
    out: an int32 [12] device tensor; info and stats are then its views [:8]
    and [8:], so that one copy brings both to the host. No host
    synchronisation here (calib mode: the tracker entry point's one read of K)."""
    for name, t in (("Xf_canon", Xf_canon), ("Cf_sum", Cf_sum), ("Xk_canon", Xk_canon), ("Ck_sum", Ck_sum)):
        _check(t, name, torch.float32)
    _check(idx_f2k, "idx_f2k", torch.int32)
    _check(valid_match, "valid_match", torch.bool)
    _check(Qk, "Qk", torch.float32)
    T_WCf, T_WCk = _poses(T_WCf, T_WCk, K)
    if K is not None and K.numel() != 9:
        raise RuntimeError("track_frame: K must be [3,3]")
    if T_WCf.numel() != 8 or T_WCk.numel() != 8:
        raise RuntimeError("track_frame: T_WCf / T_WCk must be [8] or [1,8]")
    HW = int(Xk_canon.shape[0])
    H, W = int(img_size[0]), int(img_size[1])
    if H < 1 or W < 1 or H * W != HW:
        raise RuntimeError(f"track_frame: img_size {H} x {W} does not hold HW = {HW} pixels")
    if Xf_canon.numel() != 3 * HW or Xk_canon.numel() != 3 * HW:
        raise RuntimeError("track_frame: Xf_canon / Xk_canon must be [HW,3]")
    for name, t in (("Cf_sum", Cf_sum), ("Ck_sum", Ck_sum), ("idx_f2k", idx_f2k),
                    ("valid_match", valid_match), ("Qk", Qk)):
        if t.numel() != HW:
            raise RuntimeError(f"track_frame: {name} must hold HW = {HW} elements (got {tuple(t.shape)})")
    Nf, Nk = int(Nf), int(Nk)
    if Nf < 1 or Nk < 1:
        raise RuntimeError("track_frame: Nf and Nk must be >= 1 (an initialised pointmap)")
    dev = Xk_canon.device
    _same_device("track_frame", (("Xf_canon", Xf_canon), ("Cf_sum", Cf_sum), ("Ck_sum", Ck_sum),
                                 ("idx_f2k", idx_f2k), ("valid_match", valid_match), ("Qk", Qk),
                                 ("T_WCf", T_WCf), ("T_WCk", T_WCk), ("K", K)), "Xk_canon", dev)
    if out is None:
        out = torch.empty(12, dtype=torch.int32, device=dev)  # written by the call's first launches
    else:
        _check(out, "out", torch.int32)
        if out.numel() != 12 or out.device != dev:
            raise RuntimeError(f"track_frame: out must be an int32 [12] tensor on {dev}")
    info, stats = out.view(-1)[:8], out.view(-1)[8:]
    out_f = torch.empty(1, 8, dtype=torch.float32, device=dev)
    out_r = torch.empty(1, 8, dtype=torch.float32, device=dev)
    ws = _caller_workspace(workspace, track_frame_workspace_size(HW), dev, "track_frame")
    Xf_g = Xk_g = valid_opt = None
    if return_prepared:
        Xf_g = torch.empty(HW, 3, dtype=torch.float32, device=dev)
        Xk_g = torch.empty(HW, 3, dtype=torch.float32, device=dev)
        valid_opt = torch.empty(HW, 1, dtype=torch.bool, device=dev)
    a = TrackFrameArgs()
    a.Xf_canon, a.Cf_sum, a.Xk_canon, a.Ck_sum = _p(Xf_canon), _p(Cf_sum), _p(Xk_canon), _p(Ck_sum)
    a.idx_f2k, a.valid_match, a.Qk = _p(idx_f2k), _p(valid_match), _p(Qk)
    a.T_WCf, a.T_WCk, a.K = _p(T_WCf), _p(T_WCk), _p(K)
    a.HW, a.Nf, a.Nk, a.height, a.width = HW, Nf, Nk, H, W
    a.C_conf, a.Q_conf = float(C_conf), float(Q_conf)
    a.pixel_border, a.z_eps = int(pixel_border), float(z_eps)
    a.sigma_a, a.sigma_b, a.huber_k = float(sigma_a), float(sigma_b), float(huber_k)
    a.max_iters, a.rel_error, a.delta_norm = int(max_iters), float(rel_error), float(delta_norm)
    a.sync_every = int(sync_every)
    a.T_WCf_out, a.T_CkCf_out, a.info, a.stats = _p(out_f), _p(out_r), _p(info), _p(stats)
    a.Xf_out, a.Xk_out, a.valid_opt_out = _p(Xf_g), _p(Xk_g), _p(valid_opt)
    a.workspace, a.workspace_bytes = _p(ws), ws.numel()
    _call("m3s_track_frame", ctypes.byref(a), _stream(dev))
    del ws  # stream-ordered by the caching allocator
    return (out_f, out_r, info, stats) + ((Xf_g, Xk_g, valid_opt) if return_prepared else ())
