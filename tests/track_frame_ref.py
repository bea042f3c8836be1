"""Plain-torch restatement of the part of the reference's FrameTracker.track
that mast3r_slam_backends.track_frame and mast3r_slam_amd.tracker.FrameTracker
put on the device: tracker.py:41-67 (the validity masks and match_frac),
:103-110 (the keyframe-selection statistics and decision), get_points_poses
(:129-154) and what it calls (constrain_points_to_ray -> backproject on the
pixel grid, geometry.py:37-42, 107-123; Frame.get_average_conf,
frame.py:102-103).

TEST INFRASTRUCTURE ONLY (tests/test_gpu_track_frame.py). Like
oracle/tracker_torch.py it restates the reference's arithmetic, operation for
operation and in its order, in this project's own words; the tests run it on
CPU tensors, where each operation is one correctly rounded IEEE fp32 operation.
"""
import torch


def ray_constrained(img_size, X, K):
    """constrain_points_to_ray on one [HW,3] pointmap: pixel n = (u, v) =
    (n % w, n // w) keeps its depth z and moves onto its ray. The order of
    backproject: ((u - cx) / fx) first, then times z; the third row is z * 1."""
    h, w = img_size
    n = torch.arange(h * w)
    u, v = (n % w).to(X.dtype), (n // w).to(X.dtype)
    dx = (u - K[0, 2]) / K[0, 0]
    dy = (v - K[1, 2]) / K[1, 1]
    z = X[:, 2]
    return torch.stack((z * dx, z * dy, z * torch.ones_like(z)), dim=-1)


def points_and_conf(Xf_canon, Cf_sum, Nf, Xk_canon, Ck_sum, Nk, idx_f2k, img_size, K=None):
    """get_points_poses without the poses and meas_k (the calib tracker forms
    meas_k on the device): -> (Xf [HW,3] gathered, Xk [HW,3], Cf [HW,1]
    gathered, Ck [HW,1]); both pointmaps are constrained before the gather."""
    Cf, Ck = Cf_sum / Nf, Ck_sum / Nk  # the average confidences: a tensor over a Python int
    Xf, Xk = Xf_canon, Xk_canon
    if K is not None:
        Xf, Xk = ray_constrained(img_size, Xf, K), ray_constrained(img_size, Xk, K)
    return Xf[idx_f2k], Xk, Cf[idx_f2k], Ck


def prepare(Xf_canon, Cf_sum, Nf, Xk_canon, Ck_sum, Nk, idx_f2k, valid_match, Qk, img_size, K, C_conf, Q_conf):
    """What track() computes between the matching and the optimisation, and the
    statistics it computes after it. idx_f2k [HW] int64, valid_match / Qk
    [HW,1]. The counts are Python ints; match_frac and match_frac_k are fp32
    tensors (an integer tensor over a Python int) and unique_frac_f a Python
    float, as in the reference."""
    Xf, Xk, Cf, Ck = points_and_conf(Xf_canon, Cf_sum.view(-1, 1), Nf, Xk_canon, Ck_sum.view(-1, 1), Nk,
                                     idx_f2k, img_size, K)
    good_q = Qk > Q_conf
    valid_opt = valid_match & (Cf > C_conf) & (Ck > C_conf) & good_q
    valid_kf = valid_match & good_q
    HW = valid_opt.numel()
    n_opt, n_kf = valid_opt.sum(), valid_kf.sum()
    n_unique = torch.unique(idx_f2k[valid_match[:, 0]]).shape[0]
    return dict(Xf=Xf.contiguous(), Xk=Xk.contiguous(), valid_opt=valid_opt, valid_kf=valid_kf,
                n_opt=int(n_opt), n_kf=int(n_kf), n_unique=int(n_unique),
                match_frac=n_opt / HW, match_frac_k=n_kf / HW, unique_frac_f=n_unique / HW)


def skip_frame(match_frac, cfg):
    """tracker.py:68: an fp32 tensor against the configured Python float."""
    return bool(match_frac < cfg["min_match_frac"])


def new_keyframe(match_frac_k, unique_frac_f, cfg):
    """tracker.py:110: Python's min of an fp32 tensor and a Python float."""
    return bool(min(match_frac_k, unique_frac_f) < cfg["match_frac_thresh"])
