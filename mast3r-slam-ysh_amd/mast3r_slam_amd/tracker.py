"""Host-side mirror of the reference tracker's pose refinement
(FrameTracker.opt_pose_ray_dist_sim3 / opt_pose_calib_sim3, tracker.py:173-266)
on top of the HIP entry points ``mast3r_slam_backends.track_rays_sim3`` /
``track_calib_sim3``.

Same arguments and return values as the reference methods: poses in and out
are Sim3 objects (``mast3r_slam_amd.sim3.Sim3``, the lietorch subset the
reference uses; ``.data`` is the same [..., 8] layout), results are
``(T_WCf, T_CkCf)``. A failed Cholesky raises ``torch.linalg.LinAlgError``
like the reference's ``torch.linalg.cholesky`` (tracker.py:167, caught at
:91-93). The whole GN loop — residuals, Huber whitening, 7x7 normal equations,
fp64 Cholesky, retraction and the reference's convergence rule
(nonlinear_optimizer.py:5-25) — runs on the device; the host reads the
convergence flag every ``sync_every`` iterations only.

``FrameTracker`` mirrors the reference class (tracker.py:12-127) for
everything after the network: matching, the pose optimisation's inputs, the
skip decision, the optimisation, the keyframe fusion and the new-keyframe
decision, on ``match_dense``, ``track_frame`` and ``fuse_pointmap`` with one
host read per frame.
"""
from __future__ import annotations

import torch

import mast3r_slam_backends as be

from . import matching
from .frame import Pointmap, fuse_tracked_points
from .sim3 import Sim3

# config/base.yaml:16-31
TRACKING_CFG = dict(max_iters=50, rel_error=1e-3, delta_norm=1e-3, huber=1.345, sigma_ray=0.003,
                    sigma_dist=1e1, sigma_pixel=1.0, sigma_depth=1e1, pixel_border=-10,
                    depth_eps=1e-6, C_conf=0.0, Q_conf=1.5, min_match_frac=0.05,
                    match_frac_thresh=0.333)


def _flat_pose(T) -> torch.Tensor:
    d = T.data if hasattr(T, "data") else T
    return d.reshape(-1, 8)[0].contiguous()


def _result(T_f, T_r, info):
    if int(info[be.INFO_SOLVE_FAIL]):
        raise torch.linalg.LinAlgError("tracker: Cholesky of the 7x7 normal equations failed")
    return Sim3(T_f), Sim3(T_r)


def opt_pose_ray_dist_sim3(Xf, Xk, T_WCf, T_WCk, Qk, valid, cfg=TRACKING_CFG, sync_every=5):
    """tracker.py:173-214. Xf [HW,3] (gathered by idx_f2k), Xk [HW,3], Qk [HW,1],
    valid [HW,1] bool; T_WCf / T_WCk Sim3 -> (T_WCf, T_CkCf)."""
    T_f, T_r, info = be.track_rays_sim3(
        Xf.contiguous(), Xk.contiguous(), _flat_pose(T_WCf), _flat_pose(T_WCk), Qk.contiguous(),
        valid.contiguous(), cfg["sigma_ray"], cfg["sigma_dist"], cfg["huber"], cfg["max_iters"],
        cfg["rel_error"], cfg["delta_norm"], sync_every=sync_every)
    return _result(T_f, T_r, info)


def opt_pose_calib_sim3(Xf, Xk, T_WCf, T_WCk, Qk, valid, meas_k, valid_meas_k, K, img_size,
                        cfg=TRACKING_CFG, sync_every=5):
    """tracker.py:216-266. Xf / Xk ray-constrained as get_points_poses leaves
    them (tracker.py:142-144); meas_k / valid_meas_k are formed on the device
    from the pixel grid and Xk exactly as get_points_poses does (:146-152), so
    the arguments are accepted for signature parity and not read."""
    del meas_k, valid_meas_k
    T_f, T_r, info = be.track_calib_sim3(
        Xf.contiguous(), Xk.contiguous(), _flat_pose(T_WCf), _flat_pose(T_WCk), Qk.contiguous(),
        valid.contiguous(), K.contiguous(), img_size, cfg["sigma_pixel"], cfg["sigma_depth"],
        cfg["huber"], cfg["max_iters"], cfg["rel_error"], cfg["delta_norm"], cfg["pixel_border"],
        cfg["depth_eps"], sync_every=sync_every)
    return _result(T_f, T_r, info)


def _rows(t, HW, width=None):
    """[H,W(,c)] / [1,H,W(,c)] / [HW,c] network output -> [HW, c] (c = 1 when
    width is None), as mast3r_match_asymmetric rearranges them (mast3r_utils.py:226-229)."""
    return t.reshape(HW, 1 if width is None else width).contiguous()


class FrameTracker:
    """The reference's FrameTracker (tracker.py:12-127) after the network.

    ``track`` takes the two pointmaps and what mast3r_asymmetric_inference
    returned for the pair (frame first, keyframe second: X [H,W,3], C [H,W],
    Q [H,W], D [H,W,F] each) and returns the reference's
    ``(new_kf, [Xk_canon, Ck_avg, Xf_canon, Cf_avg, Qkf, Qff], try_reloc)``.

    One host read per frame: the matching (match_dense), the frame's pointmap
    update, the optimisation's inputs, valid_opt, the three counts and the
    pose optimisation itself (track_frame, sync_every = 0) are queued without
    a synchronisation; info and stats then come to the host in one copy, and
    the skip / Cholesky / new-keyframe decisions are taken from the integer
    counts with the reference's own expressions. The price of the single read:
    on a skipped frame the optimisation has already run on the device and its
    result is discarded (the reference decides before it optimises,
    tracker.py:67-70). Nothing the frame or the keyframe holds has been touched
    by then except the frame's own pointmap, as in the reference. (With K the
    calib tracker entry point reads K back once before its launches.)"""

    def __init__(self, cfg=TRACKING_CFG, matching_cfg=matching.MATCHING_CFG):
        self.cfg = cfg
        self.matching_cfg = matching_cfg
        self._out = None
        self.reset_idx_f2k()

    def reset_idx_f2k(self):  # tracker.py:25-26
        self.idx_f2k = None

    def track(self, frame: Pointmap, keyframe: Pointmap, Xff, Cff, Qff, Dff, Xkf, Ckf, Qkf, Dkf, K=None):
        cfg = self.cfg
        H, W = (int(x) for x in Xff.shape[-3:-1])
        HW = H * W
        dev = Xff.device
        # tracker.py:31-41: idx_f2k, valid_match_k and Qk = sqrt(Qff[idx_f2k] * Qkf)
        idx, valid_match, Qk, _ = matching.match_dense(
            Xff.reshape(1, H, W, 3), Xkf.reshape(1, H, W, 3), Dff.reshape(1, H, W, -1),
            Dkf.reshape(1, H, W, -1), Qff.reshape(1, HW), Qkf.reshape(1, HW), self.idx_f2k,
            cfg=self.matching_cfg, Q_conf=cfg["Q_conf"])
        self.idx_f2k = idx.long()  # what idx_1_to_2_init accepts
        Xff, Cff, Qff = _rows(Xff, HW, 3), _rows(Cff, HW), _rows(Qff, HW)
        Xkf, Ckf, Qkf = _rows(Xkf, HW, 3), _rows(Ckf, HW), _rows(Qkf, HW)
        frame.update_pointmap(Xff, Cff)  # :44
        if self._out is None or self._out.device != dev:
            self._out = torch.empty(12, dtype=torch.int32, device=dev)
        calib = K is not None
        T_f, T_r, _, _ = be.track_frame(  # info and stats are views of self._out
            frame.X_canon, frame.C, frame.N, keyframe.X_canon, keyframe.C, keyframe.N,
            idx[0], valid_match[0], Qk[0], _flat_pose(frame.T_WC), _flat_pose(keyframe.T_WC),
            K.contiguous() if calib else None, (H, W), cfg["C_conf"], cfg["Q_conf"],
            cfg["sigma_pixel" if calib else "sigma_ray"], cfg["sigma_depth" if calib else "sigma_dist"],
            cfg["huber"], cfg["max_iters"], cfg["rel_error"], cfg["delta_norm"],
            pixel_border=cfg["pixel_border"] if calib else 0, z_eps=cfg["depth_eps"] if calib else 0.0,
            sync_every=0, out=self._out)
        host = self._out.cpu()  # the one host read of the call: info[8] and stats[4] together
        n_opt, n_kf, n_unique = (int(host[8 + k]) for k in (be.STAT_N_OPT, be.STAT_N_KF, be.STAT_N_UNIQUE))
        # :67-70, the reference's expression: an integer tensor over an int, compared in fp32
        match_frac = torch.tensor(n_opt) / HW
        if match_frac < cfg["min_match_frac"] or int(host[be.INFO_SOLVE_FAIL]):  # :68-70, :91-93
            return False, [], True
        frame.T_WC = Sim3(T_f)
        fuse_tracked_points(keyframe, T_r, Xkf, Ckf)  # :98-99
        # :104-110
        match_frac_k = torch.tensor(n_kf) / HW
        unique_frac_f = n_unique / HW
        new_kf = bool(min(match_frac_k, unique_frac_f) < cfg["match_frac_thresh"])
        if new_kf:
            self.reset_idx_f2k()
        return (new_kf, [keyframe.X_canon, keyframe.get_average_conf(), frame.X_canon,
                         frame.get_average_conf(), Qkf, Qff], False)
