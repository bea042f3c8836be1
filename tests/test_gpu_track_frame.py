"""GPU checks of track_frame (mast3r_slam_backends.track_frame ->
m3s_track_frame, csrc/gn/track_frame.h) and of mast3r_slam_amd.tracker.FrameTracker.

References:

* the reference's own outputs, tests/golden/tracker_*.npz: the prepared Xf / Xk
  its get_points_poses produced (bit for bit; in calib mode this pins
  constrain_points_to_ray) and its final poses, at the tolerance
  tests/test_gpu_tracker.py applies to the same fixtures
  (1e-5 + 1e-4 * sum of GN step lengths, identical iteration count);
* the composed path: tests/track_frame_ref.py (plain torch on CPU tensors) for
  the prepared rows, valid_opt and the counts, torch.unique included, then the
  existing track_rays_sim3 / track_calib_sim3 on its tensors. track_frame runs
  the same kernels on the same inputs, so poses and info are bit-identical and
  the counts are equal integers;
* for FrameTracker.track, the reference's sequence driven with the existing
  matching.match_dense, opt_pose_* and fuse_tracked_points.

Shapes: 64x48 and 32x24 (the fixtures' sizes; 12 and 3 workgroups of the prep
kernel), 9x7 = 63 and 33x31 = 1023 pixels (a partial last wave, a map whose
last 16-byte word is partial).
"""
import functools
import os

import numpy as np
import pytest
import torch

import track_frame_ref as ref

pytestmark = pytest.mark.gpu

from oracle import tracker_oracle as tro  # noqa: E402

DEV = torch.device("cuda:0")
CFG = dict(tro.TRACKING_CFG)  # C_conf = 0.0, Q_conf = 1.5 (config/base.yaml tracking)


@pytest.fixture(scope="module")
def be():
    import mast3r_slam_backends as be

    return be


def pose_tol(taus):  # tests/test_gpu_tracker.py
    return 1e-5 + 1e-4 * float(np.linalg.norm(np.asarray(taus, np.float64), axis=-1).sum())


def _bits(t):
    return t.contiguous().view(torch.int32)


def run_frame(be, ins, cfg=CFG, max_iters=None, workspace=None):
    """track_frame on the CPU tensors of ins (idx int64) -> CPU results."""
    d = lambda k: ins[k].to(DEV)  # noqa: E731
    K = ins.get("K")
    calib = K is not None
    out = be.track_frame(
        d("Xf_canon"), d("Cf_sum"), ins["Nf"], d("Xk_canon"), d("Ck_sum"), ins["Nk"], d("idx").int(),
        d("valid_match"), d("Qk"), d("T_WCf"), d("T_WCk"), K.to(DEV) if calib else None, ins["img_size"],
        cfg["C_conf"], cfg["Q_conf"], cfg["sigma_pixel" if calib else "sigma_ray"],
        cfg["sigma_depth" if calib else "sigma_dist"], cfg["huber"],
        cfg["max_iters"] if max_iters is None else max_iters, cfg["rel_error"], cfg["delta_norm"],
        pixel_border=cfg["pixel_border"] if calib else 0, z_eps=cfg["depth_eps"] if calib else 0.0,
        sync_every=0, workspace=workspace, return_prepared=True)
    torch.cuda.synchronize()
    names = ("T_WCf", "T_CkCf", "info", "stats", "Xf", "Xk", "valid_opt")
    return dict(zip(names, (o.cpu() for o in out)))


def run_ref(ins, cfg=CFG):
    return ref.prepare(ins["Xf_canon"], ins["Cf_sum"], ins["Nf"], ins["Xk_canon"], ins["Ck_sum"], ins["Nk"],
                       ins["idx"], ins["valid_match"], ins["Qk"], ins["img_size"], ins.get("K"),
                       cfg["C_conf"], cfg["Q_conf"])


def run_composed(be, ins, prep, cfg=CFG, max_iters=None):
    """The existing tracker entry points on the restatement's tensors."""
    d = lambda t: t.to(DEV)  # noqa: E731
    mi = cfg["max_iters"] if max_iters is None else max_iters
    if ins.get("K") is not None:
        out = be.track_calib_sim3(d(prep["Xf"]), d(prep["Xk"]), d(ins["T_WCf"]), d(ins["T_WCk"]), d(ins["Qk"]),
                                  d(prep["valid_opt"]), d(ins["K"]), ins["img_size"], cfg["sigma_pixel"],
                                  cfg["sigma_depth"], cfg["huber"], mi, cfg["rel_error"], cfg["delta_norm"],
                                  cfg["pixel_border"], cfg["depth_eps"], sync_every=0)
    else:
        out = be.track_rays_sim3(d(prep["Xf"]), d(prep["Xk"]), d(ins["T_WCf"]), d(ins["T_WCk"]), d(ins["Qk"]),
                                 d(prep["valid_opt"]), cfg["sigma_ray"], cfg["sigma_dist"], cfg["huber"], mi,
                                 cfg["rel_error"], cfg["delta_norm"], sync_every=0)
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def assert_prepared(got, prep):
    assert torch.equal(_bits(got["Xf"]), _bits(prep["Xf"]))
    assert torch.equal(_bits(got["Xk"]), _bits(prep["Xk"]))
    assert got["valid_opt"].dtype == torch.bool and torch.equal(got["valid_opt"], prep["valid_opt"])


def assert_counts(got, prep):
    assert got["stats"].dtype == torch.int32
    assert got["stats"].tolist() == [prep["n_opt"], prep["n_kf"], prep["n_unique"], 0]


def assert_same_as_composed(be, ins, got, prep, cfg=CFG, max_iters=None):
    T_f, T_r, info = run_composed(be, ins, prep, cfg, max_iters)
    assert torch.equal(got["info"], info)
    assert torch.equal(_bits(got["T_WCf"]), _bits(T_f)) and torch.equal(_bits(got["T_CkCf"]), _bits(T_r))


# ------------------------------------------------ the reference's fixtures --
@pytest.mark.parametrize("name", ["tracker_rays_64x48", "tracker_calib_64x48", "tracker_rays_identity_64x48",
                                  "tracker_calib_identity_64x48"])
def test_pinned_to_reference_fixture(be, golden_dir, name):
    d = dict(np.load(os.path.join(golden_dir, name + ".npz")))
    t = lambda k: torch.from_numpy(np.ascontiguousarray(d[k]))  # noqa: E731
    H, W = int(d["H"]), int(d["W"])
    HW = H * W
    ins = dict(Xf_canon=t("Xf_raw"), Cf_sum=torch.full((HW, 1), 2.0), Nf=1, Xk_canon=t("Xk_raw"),
               Ck_sum=torch.full((HW, 1), 3.0), Nk=1, idx=torch.arange(HW), valid_match=t("valid"), Qk=t("Qk"),
               T_WCf=t("T_WCf_init"), T_WCk=t("T_WCk"), img_size=(H, W), K=t("K") if int(d["calib"]) else None)
    got = run_frame(be, ins, max_iters=int(d["max_iters"]))
    assert torch.equal(_bits(got["Xf"]), _bits(t("Xf")))  # the reference's get_points_poses, bit for bit
    assert torch.equal(_bits(got["Xk"]), _bits(t("Xk")))
    assert torch.equal(got["valid_opt"], t("valid"))
    n = int(d["valid"].sum())
    assert got["stats"].tolist() == [n, n, n, 0]
    info = got["info"].numpy()
    assert info[1] == 0 and info[0] == int(d["n_iters"])
    tol = pose_tol(d["tau_iter"])
    np.testing.assert_allclose(got["T_WCf"].numpy()[0], d["T_WCf"][0], atol=tol)
    np.testing.assert_allclose(got["T_CkCf"].numpy()[0], d["T_CkCf"][0], atol=tol)


def test_all_invalid_reports_failed_solve(be, golden_dir):
    d = dict(np.load(os.path.join(golden_dir, "tracker_rays_allinvalid_32x24.npz")))
    t = lambda k: torch.from_numpy(np.ascontiguousarray(d[k]))  # noqa: E731
    H, W = int(d["H"]), int(d["W"])
    HW = H * W
    assert int(d["valid"].sum()) == 0
    ins = dict(Xf_canon=t("Xf_raw"), Cf_sum=torch.full((HW, 1), 2.0), Nf=1, Xk_canon=t("Xk_raw"),
               Ck_sum=torch.full((HW, 1), 2.0), Nk=1, idx=torch.arange(HW), valid_match=t("valid"), Qk=t("Qk"),
               T_WCf=t("T_WCf_init"), T_WCk=t("T_WCk"), img_size=(H, W))
    got = run_frame(be, ins, max_iters=int(d["max_iters"]))
    assert got["stats"].tolist() == [0, 0, 0, 0]
    assert not got["valid_opt"].any()
    assert got["info"][1] == 1  # the reference raises -> track() reports failure
    assert_same_as_composed(be, ins, got, run_ref(ins), max_iters=int(d["max_iters"]))


# ------------------------------------------------------ the composed path --
@functools.lru_cache(maxsize=None)
def _pair_inputs(H, W, calib, seed=1201):
    """A synthetic pair with a near-identity idx that repeats pixels, update
    counts Nf = 3 and Nk = 2, confidences on both sides of C_conf = 3.0, and
    matches marked valid whose Qk is below Q_conf (make_pair's valid holds
    Qk > 1.5 already; three in ten of the others are switched on). CPU tensors,
    never modified by a test."""
    from mast3r_slam_amd import synthetic

    p = synthetic.make_pair(H, W, seed=seed)
    HW = H * W
    gen = torch.Generator().manual_seed(seed + 1)
    idx = (torch.arange(HW) + torch.randint(-2, 3, (HW,), generator=gen)).clamp_(0, HW - 1)
    idx[5::11] = idx[4::11][: idx[5::11].numel()]  # exact repeats of a neighbour's target
    valid_match = p.valid | (torch.rand(HW, 1, generator=gen) < 0.3)
    return dict(Xf_canon=p.Xf, Cf_sum=(p.Cf * 3.0).contiguous(), Nf=3, Xk_canon=p.Xk,
                Ck_sum=(p.Ck * 2.0).contiguous(), Nk=2, idx=idx, valid_match=valid_match, Qk=p.Qk,
                T_WCf=p.T_WCf_init.data.clone(), T_WCk=p.T_WCk.data.clone(), img_size=(H, W),
                K=p.K if calib else None)


CFG_C3 = dict(CFG, C_conf=3.0)


@pytest.mark.parametrize("calib", [False, True], ids=["rays", "calib"])
@pytest.mark.parametrize("H,W", [(48, 64), (24, 32)])
def test_equals_composed_path(be, H, W, calib):
    ins = _pair_inputs(H, W, calib)
    prep = run_ref(ins, CFG_C3)
    HW = H * W
    assert prep["n_unique"] < int(ins["valid_match"].sum())  # idx repeats pixels
    assert 0.05 * HW < prep["n_opt"] < prep["n_kf"] < int(ins["valid_match"].sum()) < HW  # every mask cuts
    got = run_frame(be, ins, CFG_C3)
    assert_prepared(got, prep)
    assert_counts(got, prep)
    assert got["info"][1] == 0 and got["info"][0] >= 1
    assert_same_as_composed(be, ins, got, prep, CFG_C3)


@pytest.mark.parametrize("H,W", [(7, 9), (31, 33)])
def test_tails_rays(be, H, W):
    """HW = 63 and 1023: the last wave and the last 16 bytes of the map are
    partial. The tracker entry points take these shapes, so track_frame does."""
    ins = _pair_inputs(H, W, False)
    assert (H * W) % 64 != 0 and (H * W) % 16 != 0
    prep = run_ref(ins)
    assert prep["n_unique"] > 1
    got = run_frame(be, ins)
    assert_prepared(got, prep)
    assert_counts(got, prep)
    assert_same_as_composed(be, ins, got, prep)


# ------------------------------------------------------------- the counts --
def _count_inputs(idx, valid_match, H=24, W=32, **over):
    ins = dict(_pair_inputs(H, W, False))
    ins.update(idx=idx, valid_match=valid_match.view(-1, 1), **over)
    return ins


def _some_valid(HW, seed):
    return torch.rand(HW, generator=torch.Generator().manual_seed(seed)) < 0.6


def test_counts_every_idx_the_same_pixel(be):
    HW = 768
    ins = _count_inputs(torch.full((HW,), 411), _some_valid(HW, 1))
    prep = run_ref(ins)
    assert prep["n_unique"] == 1 and prep["n_kf"] > 1
    got = run_frame(be, ins)
    assert_counts(got, prep)
    assert_prepared(got, prep)


def test_counts_permutation(be):
    HW = 768
    valid = _some_valid(HW, 2)
    ins = _count_inputs(torch.randperm(HW, generator=torch.Generator().manual_seed(3)), valid)
    prep = run_ref(ins)
    assert prep["n_unique"] == int(valid.sum())
    got = run_frame(be, ins)
    assert_counts(got, prep)
    assert_prepared(got, prep)


def test_counts_duplicates_only_among_invalid_matches(be):
    """Pixels without a valid match point at a valid pixel's target or at a
    target nothing valid points at: neither may be counted."""
    HW = 768
    valid = _some_valid(HW, 4)
    valid[:2] = torch.tensor([True, False])
    idx = torch.arange(HW)
    inv = (~valid).nonzero()[:, 0]
    idx[inv[0::2]] = 0  # pixel 0 is valid and points at 0: a duplicate of a counted target
    idx[inv[1::2]] = 1  # pixel 1 is invalid: target 1 is hit by invalid matches only
    ins = _count_inputs(idx, valid)
    prep = run_ref(ins)
    assert prep["n_unique"] == int(valid.sum())
    got = run_frame(be, ins)
    assert_counts(got, prep)


def _around(x):
    """float32 x and its two neighbours, ascending."""
    x = np.float32(x)
    return [float(np.nextafter(x, np.float32(-np.inf))), float(x), float(np.nextafter(x, np.float32(np.inf)))]


def test_counts_values_exactly_at_the_thresholds(be):
    """Qk, Cf_sum / 3 and Ck_sum / 2 below, at and above their thresholds in
    every combination: the comparisons are strict, and Cf_sum / Nf is a true
    fp32 division (5.1f / 3 is not 5.1f * (1/3.f))."""
    HW = 768
    s = np.float32(5.1)
    c = np.float32(s / np.float32(3.0))  # C_conf: the correctly rounded quotient
    assert np.float32(s * np.float32(1.0 / 3.0)) != c  # a multiply by the reciprocal lands elsewhere
    cf = torch.tensor(_around(s))  # / 3 -> below, at, above c
    ck = torch.tensor(_around(np.float32(2.0) * c))  # / 2 -> exactly the neighbours of c
    q = torch.tensor(_around(1.5))
    assert [(x / 3 > float(c)).item() for x in cf] == [False, False, True] and (cf[1] / 3).item() == float(c)
    n = torch.arange(HW)
    ins = _count_inputs(n.flip(0).contiguous(), torch.ones(HW, dtype=torch.bool),
                        Ck_sum=ck[n % 3].view(-1, 1), Nk=2, Cf_sum=cf[(n // 3) % 3].flip(0).view(-1, 1), Nf=3,
                        Qk=q[(n // 9) % 3].view(-1, 1))
    cfg = dict(CFG, C_conf=float(c), Q_conf=1.5)
    prep = run_ref(ins, cfg)
    top_q, top_cf, top_ck = (n // 9) % 3 == 2, (n // 3) % 3 == 2, n % 3 == 2  # strictly above only
    assert prep["n_kf"] == int(top_q.sum()) == 252
    assert prep["n_opt"] == int((top_q & top_cf & top_ck).sum()) == 28
    got = run_frame(be, ins, cfg)
    assert_counts(got, prep)
    assert_prepared(got, prep)


def test_no_state_carried_between_calls(be):
    """Two calls on one caller-owned workspace that starts as 0xFF bytes; the
    second has fewer distinct targets, so a map or a counter left by the first
    would show."""
    HW = 768
    valid = _some_valid(HW, 5)
    first = _count_inputs(torch.randperm(HW, generator=torch.Generator().manual_seed(6)), valid)
    second = _count_inputs(torch.arange(HW) % 7, valid)
    ws = torch.full((be.track_frame_workspace_size(HW),), 0xFF, dtype=torch.uint8, device=DEV)
    for ins in (first, second):
        fresh = run_frame(be, ins)
        got = run_frame(be, ins, workspace=ws)
        prep = run_ref(ins)
        assert_counts(fresh, prep)
        assert_counts(got, prep)
        for k in fresh:
            assert torch.equal(got[k], fresh[k]), k
    assert run_ref(second)["n_unique"] == 7 < run_ref(first)["n_unique"]


def test_bad_inputs_raise(be):
    ins = _pair_inputs(24, 32, False)
    HW = 768
    with pytest.raises(RuntimeError, match="idx_f2k"):  # int64, as matching.match returns it
        be.track_frame(*_positional(ins, idx=ins["idx"].to(DEV)))
    with pytest.raises(RuntimeError, match="img_size"):
        be.track_frame(*_positional(ins, img_size=(24, 33)))
    with pytest.raises(RuntimeError, match="Qk"):
        be.track_frame(*_positional(ins, Qk=ins["Qk"][:-1].contiguous().to(DEV)))
    with pytest.raises(RuntimeError, match="Xf_canon"):
        be.track_frame(*_positional(ins, Xf_canon=ins["Xf_canon"].double().to(DEV)))
    with pytest.raises(RuntimeError, match="workspace"):
        be.track_frame(*_positional(ins), workspace=torch.empty(be.track_frame_workspace_size(HW) - 1,
                                                                dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="Nf"):
        be.track_frame(*_positional(ins, Nf=0))


def _positional(ins, **over):
    d = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in ins.items()}
    d["idx"] = d["idx"].int()
    d.update(over)
    return (d["Xf_canon"], d["Cf_sum"], d["Nf"], d["Xk_canon"], d["Ck_sum"], d["Nk"], d["idx"], d["valid_match"],
            d["Qk"], d["T_WCf"], d["T_WCk"], d["K"], d["img_size"], CFG["C_conf"], CFG["Q_conf"], CFG["sigma_ray"],
            CFG["sigma_dist"], CFG["huber"], 5, CFG["rel_error"], CFG["delta_norm"])


# ------------------------------------------------------ FrameTracker.track --
TH, TW = 48, 64


@functools.lru_cache(maxsize=None)
def _net_outputs():
    """What mast3r_asymmetric_inference returns for a (frame, keyframe) pair at
    64x48, and the keyframe's own pointmap: CPU tensors, never modified. The
    frame is view 1 of synthetic.make_match_inputs, the keyframe view 2; Xkf is
    the keyframe's pointmap in the frame's camera (X21). Descriptor confidences
    as tests/test_gpu_match_dense.py builds them: uniform in [1, 3]."""
    from mast3r_slam_amd import synthetic
    from mast3r_slam_amd.sim3 import Sim3

    m = synthetic.make_match_inputs(TH, TW, seed=1005)
    HW = TH * TW
    gen = torch.Generator().manual_seed(1006)
    Qff = 1.0 + 2.0 * torch.rand(TH, TW, generator=gen)
    Qkf = 1.0 + 2.0 * torch.rand(TH, TW, generator=gen)
    Cff = 1.0 + torch.exp(1.0 + 0.5 * torch.randn(TH, TW, generator=gen))
    Ckf = 1.0 + torch.exp(1.0 + 0.5 * torch.randn(TH, TW, generator=gen))
    T = synthetic.loop_trajectory(16, None)[0:2]  # the poses make_match_inputs uses: frame, keyframe
    T_WCf, T_WCk = Sim3(T.data[0:1].clone()), Sim3(T.data[1:2].clone())
    Xk_canon = (T_WCk.inv() * T_WCf).act(m.X21.reshape(HW, 3)).contiguous()
    Ck_sum = 2.0 * (1.0 + torch.exp(1.0 + 0.5 * torch.randn(HW, 1, generator=gen)))  # N = 2
    xi = torch.zeros(1, 7)
    xi[:, 0:3] = torch.randn(1, 3, generator=gen) * 0.02
    xi[:, 3:6] = torch.randn(1, 3, generator=gen) * 0.0175
    T_WCf_init = Sim3.exp(xi) * T_WCf
    K = synthetic.intrinsics(TH, TW)
    return dict(Xff=m.X11[0], Cff=Cff, Qff=Qff, Dff=m.D11[0], Xkf=m.X21[0], Ckf=Ckf, Qkf=Qkf,
                Dkf=m.D21[0].reshape(TH, TW, -1), Xk_canon=Xk_canon, Ck_sum=Ck_sum,
                T_WCf_init=T_WCf_init.data, T_WCk=T_WCk.data, K=K)


def _pointmaps(net, Ck_sum=None):
    from mast3r_slam_amd.frame import Pointmap
    from mast3r_slam_amd.sim3 import Sim3

    frame, keyframe = Pointmap(), Pointmap()
    frame.T_WC = Sim3(net["T_WCf_init"].to(DEV))
    keyframe.T_WC = Sim3(net["T_WCk"].to(DEV))
    keyframe.X_canon = net["Xk_canon"].to(DEV)
    keyframe.C = (net["Ck_sum"] if Ck_sum is None else Ck_sum).to(DEV)
    keyframe.N = keyframe.N_updates = 2
    return frame, keyframe


def _net_args(net):
    return [net[k].to(DEV) for k in ("Xff", "Cff", "Qff", "Dff", "Xkf", "Ckf", "Qkf", "Dkf")]


def reference_track(frame, keyframe, idx_init, Xff, Cff, Qff, Dff, Xkf, Ckf, Qkf, Dkf, K, cfg):
    """tracker.py:28-127 with the existing entry points and the restatement:
    -> ((new_kf, list, try_reloc), the idx_f2k the tracker keeps)."""
    from mast3r_slam_amd import matching, tracker
    from mast3r_slam_amd.frame import fuse_tracked_points

    HW = TH * TW
    idx, valid, Qk, _ = matching.match_dense(Xff[None], Xkf[None], Dff[None], Dkf[None], Qff.reshape(1, HW),
                                             Qkf.reshape(1, HW), idx_init, Q_conf=cfg["Q_conf"])
    kept = idx.long()
    Xff, Cff, Qff = Xff.reshape(HW, 3), Cff.reshape(HW, 1), Qff.reshape(HW, 1)
    Xkf, Ckf, Qkf = Xkf.reshape(HW, 3), Ckf.reshape(HW, 1), Qkf.reshape(HW, 1)
    frame.update_pointmap(Xff, Cff)
    prep = ref.prepare(frame.X_canon.cpu(), frame.C.cpu(), frame.N, keyframe.X_canon.cpu(), keyframe.C.cpu(),
                       keyframe.N, kept[0].cpu(), valid[0].cpu(), Qk[0].cpu(), (TH, TW),
                       None if K is None else K.cpu(), cfg["C_conf"], cfg["Q_conf"])
    if ref.skip_frame(prep["match_frac"], cfg):
        return (False, [], True), kept, prep
    Xf, Xk, valid_opt = prep["Xf"].to(DEV), prep["Xk"].to(DEV), prep["valid_opt"].to(DEV)
    try:
        if K is None:
            T_WCf, T_CkCf = tracker.opt_pose_ray_dist_sim3(Xf, Xk, frame.T_WC, keyframe.T_WC, Qk[0], valid_opt,
                                                           cfg=cfg, sync_every=0)
        else:
            T_WCf, T_CkCf = tracker.opt_pose_calib_sim3(Xf, Xk, frame.T_WC, keyframe.T_WC, Qk[0], valid_opt, None,
                                                        None, K, (TH, TW), cfg=cfg, sync_every=0)
    except torch.linalg.LinAlgError:
        return (False, [], True), kept, prep
    frame.T_WC = T_WCf
    fuse_tracked_points(keyframe, T_CkCf, Xkf, Ckf)
    new_kf = ref.new_keyframe(prep["match_frac_k"], prep["unique_frac_f"], cfg)
    if new_kf:
        kept = None
    return (new_kf, [keyframe.X_canon, keyframe.get_average_conf(), frame.X_canon, frame.get_average_conf(),
                     Qkf, Qff], False), kept, prep


def _assert_track_equal(got, want, ft, kept, frame, frame_r, keyframe, keyframe_r):
    assert got[0] == want[0]
    assert got[2] == want[2] and len(got[1]) == len(want[1])
    for a, b in zip(got[1], want[1]):
        assert a.shape == b.shape and torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(frame.T_WC.data), _bits(frame_r.T_WC.data))
    assert torch.equal(_bits(keyframe.X_canon), _bits(keyframe_r.X_canon))
    assert torch.equal(_bits(keyframe.C), _bits(keyframe_r.C)) and keyframe.N == keyframe_r.N
    assert torch.equal(_bits(frame.X_canon), _bits(frame_r.X_canon)) and frame.N == frame_r.N
    if kept is None:
        assert ft.idx_f2k is None
    else:
        assert ft.idx_f2k.dtype == torch.int64 and torch.equal(ft.idx_f2k, kept)


@pytest.mark.parametrize("calib", [False, True], ids=["rays", "calib"])
def test_frame_tracker_normal_frame(calib):
    """Two frames in a row (the second starts from the stored idx_f2k) with the
    keyframe threshold below and then above the statistics, so that both
    values of new_kf and the idx reset are seen."""
    from mast3r_slam_amd import tracker

    net = _net_outputs()
    K = net["K"].to(DEV) if calib else None
    seen = []
    for thresh in (0.05, 0.999):
        cfg = dict(tracker.TRACKING_CFG, match_frac_thresh=thresh)
        ft = tracker.FrameTracker(cfg)
        kept = None
        keyframe, keyframe_r = _pointmaps(net)[1], _pointmaps(net)[1]
        for _ in range(2):
            frame, frame_r = _pointmaps(net)[0], _pointmaps(net)[0]
            want, kept, prep = reference_track(frame_r, keyframe_r, kept, *_net_args(net), K, cfg)
            got = ft.track(frame, keyframe, *_net_args(net), K=K)
            assert want[2] is False and prep["n_opt"] > 0.1 * TH * TW
            _assert_track_equal(got, want, ft, kept, frame, frame_r, keyframe, keyframe_r)
            assert keyframe.N == keyframe_r.N
        seen.append(got[0])
        assert keyframe.N == 4
    assert seen == [False, True]


def test_frame_tracker_skipped_frame():
    """No keyframe confidence above C_conf -> match_frac = 0 < min_match_frac:
    (False, [], True), keyframe and frame pose untouched."""
    from mast3r_slam_amd import tracker

    net = _net_outputs()
    zero = torch.zeros_like(net["Ck_sum"])
    frame, keyframe = _pointmaps(net, zero)
    X0, C0, T0 = keyframe.X_canon.clone(), keyframe.C.clone(), frame.T_WC
    ft = tracker.FrameTracker()
    got = ft.track(frame, keyframe, *_net_args(net))
    assert got == (False, [], True)
    assert torch.equal(_bits(keyframe.X_canon), _bits(X0)) and torch.equal(_bits(keyframe.C), _bits(C0))
    assert keyframe.N == 2 and keyframe.N_updates == 2
    assert frame.T_WC is T0 and torch.equal(_bits(T0.data), _bits(net["T_WCf_init"].to(DEV)))
    assert ft.idx_f2k is not None  # tracker.py:35: saved before the decision


@pytest.mark.parametrize("n_opt", [153, 154])
def test_frame_tracker_min_match_frac_boundary(n_opt):
    """HW = 3072: 153 / 3072 and 154 / 3072 are the fp32 quotients nearest to
    float32(0.05) = 0.0500000007 from below and above. The keyframe's
    confidence is positive on exactly n_opt of the pixels with a valid match
    and Qk > Q_conf, so n_opt is the count of valid_opt."""
    from mast3r_slam_amd import matching, tracker

    net = _net_outputs()
    HW = TH * TW
    cfg = tracker.TRACKING_CFG
    lo, hi = torch.tensor(153) / HW, torch.tensor(154) / HW
    assert lo < cfg["min_match_frac"] and not hi < cfg["min_match_frac"]
    a = _net_args(net)
    _, valid, Qk, _ = matching.match_dense(a[0][None], a[4][None], a[3][None], a[7][None], a[2].reshape(1, HW),
                                           a[6].reshape(1, HW), Q_conf=cfg["Q_conf"])
    good = (valid[0, :, 0] & (Qk[0, :, 0] > cfg["Q_conf"])).cpu().nonzero()[:, 0]
    assert good.numel() >= 154
    Ck_sum = torch.zeros(HW, 1)
    Ck_sum[good[(torch.arange(n_opt) * good.numel()) // n_opt]] = 2.5  # n_opt of them, spread over the image
    frame, keyframe = _pointmaps(net, Ck_sum)
    frame_r, keyframe_r = _pointmaps(net, Ck_sum)
    want, kept, prep = reference_track(frame_r, keyframe_r, None, *a, None, cfg)
    assert prep["n_opt"] == n_opt
    assert want[2] is (n_opt == 153)  # skipped below the threshold, tracked above it
    ft = tracker.FrameTracker()
    got = ft.track(frame, keyframe, *a)
    if want[2]:
        assert got == (False, [], True) and keyframe.N == 2
        assert torch.equal(_bits(keyframe.X_canon), _bits(keyframe_r.X_canon))
    else:
        _assert_track_equal(got, want, ft, kept, frame, frame_r, keyframe, keyframe_r)
