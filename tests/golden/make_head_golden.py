"""Writes tests/golden/head_{a..e}.npz from the reference's own catmlp+dpt head.

    python tests/golden/make_head_golden.py <reference checkout>

It needs the reference's source tree and runs only where that is present; the
tests read the fixtures it leaves. Two files are loaded from their paths:
<reference>/thirdparty/mast3r/dust3r/dust3r/heads/postprocess.py (it imports
only torch) and <reference>/thirdparty/mast3r/mast3r/catmlp_dpt_head.py, the
latter with dust3r.heads.dpt_head, models.blocks and the two path_to_* modules
stubbed in sys.modules (they are the network, which is not run here). A head
object is made without its constructor: its `dpt` and `head_local_features`
return the seeded raw maps, so the reference's own forward runs its transpose /
view / F.pixel_shuffle / cat / postprocess on them, on the CPU in fp32.

Every fixture stores `pts` [B,4,H,W] f32, `feat` [B,S,(F+1)*P*P] f32, `P`, `F`,
`conf` and `desc_conf` (vmin, vmax), and the reference's `pts3d` [B,H,W,3],
`conf_out` [B,H,W], `desc` [B,H,W,F], `desc_conf_out` [B,H,W].
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
INF = float("inf")

#        B   H   W   P   F  conf        desc_conf   spread
CASES = {
    "a": (2, 32, 48, 16, 24, (1.0, INF), (0.0, INF), False),  # the released shape class, several tokens, two images
    "b": (1, 16, 16, 16, 24, (1.0, INF), (0.0, INF), False),  # one token
    "c": (1, 12, 20, 4, 5, (1.0, INF), (0.0, INF), False),    # generic: small patch, odd F
    "d": (1, 6, 10, 2, 3, (1.0, 5.0), (0.5, 3.0), False),     # generic, and both clips finite
    "e": (1, 16, 32, 16, 24, (1.0, INF), (0.0, INF), True),   # d from 1e-9 to 20, raw confidences from -30 to 30
}


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(ref_root):
    mast3r = os.path.join(ref_root, "thirdparty", "mast3r")
    for name in ("mast3r", "mast3r.utils", "mast3r.utils.path_to_dust3r", "dust3r", "dust3r.heads", "dust3r.utils",
                 "dust3r.utils.path_to_croco", "models"):
        sys.modules[name] = types.ModuleType(name)
    dpt = types.ModuleType("dust3r.heads.dpt_head")
    dpt.PixelwiseTaskWithDPT = torch.nn.Module
    sys.modules["dust3r.heads.dpt_head"] = dpt
    blocks = types.ModuleType("models.blocks")
    blocks.Mlp = torch.nn.Module
    sys.modules["models.blocks"] = blocks
    _load("dust3r.heads.postprocess", os.path.join(mast3r, "dust3r", "dust3r", "heads", "postprocess.py"))
    return _load("reference_catmlp_dpt_head", os.path.join(mast3r, "mast3r", "catmlp_dpt_head.py"))


def raw_inputs(rng, B, H, W, P, F, spread):
    S, PP = (H // P) * (W // P), P * P
    pts = rng.standard_normal((B, 4, H, W))
    feat = rng.standard_normal((B, S, (F + 1) * PP))
    pts[:, 3] *= 2.0
    feat[:, :, F * PP:] *= 2.0
    if spread:
        direction = pts[:, :3] / np.sqrt((pts[:, :3] ** 2).sum(1, keepdims=True))
        pts[:, :3] = direction * np.exp(rng.uniform(np.log(1e-9), np.log(20.0), (B, 1, H, W)))
        pts[:, 3] = rng.uniform(-30.0, 30.0, (B, H, W))
        feat[:, :, F * PP:] = rng.uniform(-30.0, 30.0, (B, S, PP))
        # descriptors of very different lengths: a factor per (token, in-patch position)
        feat[:, :, :F * PP] *= np.tile(np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (B, S, PP))), (1, 1, F))
    return pts.astype(np.float32), feat.astype(np.float32)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    for k, (name, (B, H, W, P, F, conf, desc_conf, spread)) in enumerate(sorted(CASES.items())):
        pts, feat = raw_inputs(np.random.RandomState(200 + k), B, H, W, P, F, spread)
        head = object.__new__(ref.Cat_MLP_LocalFeatures_DPT_Pts3d)
        torch.nn.Module.__init__(head)
        head.dpt = lambda decout, image_size, _p=pts: torch.from_numpy(_p)
        head.head_local_features = lambda cat, _f=feat: torch.from_numpy(_f)
        head.patch_size, head.local_feat_dim, head.two_confs, head.desc_mode = P, F, True, "norm"
        head.depth_mode, head.conf_mode, head.desc_conf_mode = ("exp", -INF, INF), ("exp", *conf), ("exp", *desc_conf)
        head.postprocess = ref.postprocess
        S = (H // P) * (W // P)
        with torch.no_grad():
            res = ref.Cat_MLP_LocalFeatures_DPT_Pts3d.forward(head, [torch.zeros(B, S, 1), torch.zeros(B, S, 1)], (H, W))
        assert tuple(res["desc"].shape) == (B, H, W, F) and res["desc"].dtype == torch.float32
        path = os.path.join(HERE, f"head_{name}.npz")
        np.savez_compressed(path, pts=pts, feat=feat, P=np.int64(P), F=np.int64(F), conf=np.float64(conf),
                            desc_conf=np.float64(desc_conf), pts3d=res["pts3d"].numpy(), conf_out=res["conf"].numpy(),
                            desc=res["desc"].numpy(), desc_conf_out=res["desc_conf"].numpy())
        print(f"{path}: B={B} H={H} W={W} P={P} F={F} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
