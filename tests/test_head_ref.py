"""tests/head_ref.py against the reference's own catmlp+dpt head (no GPU needed):
for every fixture of tests/golden/make_head_golden.py the reference's fp32
outputs lie within head_ref.bounds of head_ref.head_exact, NaN and inf by class
and position. That pins the restatement's pixel_shuffle indexing, channel order
and modes to the reference's code, and shows that the bound is not tighter than
the reference's own arithmetic; a wrong unshuffle is off by O(1), so the bound
can tell."""
import os

import numpy as np
import pytest
import torch

import head_ref

FIXTURES = ("a", "b", "c", "d", "e")
OUT = {"X": "pts3d", "C": "conf_out", "D": "desc", "Q": "desc_conf_out"}


def load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, f"head_{name}.npz"))
    fx = {k: z[k] for k in z.files}
    fx["P"], fx["F"] = int(fx["P"]), int(fx["F"])
    fx["conf"], fx["desc_conf"] = tuple(float(v) for v in fx["conf"]), tuple(float(v) for v in fx["desc_conf"])
    return fx


def test_fixture_set_is_the_one_the_kernel_needs(golden_dir):
    shapes = {}
    for name in FIXTURES:
        fx = load(golden_dir, name)
        B, _, H, W = fx["pts"].shape
        shapes[name] = (B, H, W, fx["P"], fx["F"])
        assert fx["pts"].dtype == fx["feat"].dtype == fx["desc"].dtype == np.float32
        assert fx["desc"].shape == (B, H, W, fx["F"]) and fx["pts3d"].shape == (B, H, W, 3)
        assert fx["conf_out"].shape == fx["desc_conf_out"].shape == (B, H, W)
    assert shapes == {"a": (2, 32, 48, 16, 24), "b": (1, 16, 16, 16, 24), "c": (1, 12, 20, 4, 5),
                      "d": (1, 6, 10, 2, 3), "e": (1, 16, 32, 16, 24)}
    e = load(golden_dir, "e")
    d = np.sqrt((e["pts"][:, :3].astype(np.float64) ** 2).sum(1))
    assert d.min() < 1e-8 and d.max() > 10.0 and d.min() >= 1e-9 * 0.99 and d.max() <= 20.0 * 1.01
    lq = head_ref.unshuffle(e["feat"], 16, 32, 16, 24)[..., 24]
    for raw in (e["pts"][:, 3], lq):
        assert raw.min() < -25.0 and raw.max() > 25.0 and np.abs(raw).max() <= 30.0
    dd = load(golden_dir, "d")  # both clips are finite and both take effect
    assert dd["conf"] == (1.0, 5.0) and dd["desc_conf"] == (0.5, 3.0)
    assert (dd["conf_out"] == 5.0).any() and (dd["conf_out"] < 5.0).any()
    assert (dd["desc_conf_out"] == 3.0).any() and (dd["desc_conf_out"] < 3.0).any()


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_within_bound_of_exact(golden_dir, name):
    fx = load(golden_dir, name)
    args = (fx["pts"], fx["feat"], fx["P"], fx["F"], fx["conf"], fx["desc_conf"])
    exact, tol = head_ref.head_exact(*args), head_ref.bounds(*args)
    for key, ref_key in OUT.items():
        ok, worst = head_ref.compare(fx[ref_key], exact[key], tol[key])
        print(f"head_{name} {key}: max |reference - exact| / bound = {worst:.3f}")
        assert ok, (key, worst)


def test_a_wrong_unshuffle_is_far_outside_the_bound(golden_dir):
    fx = load(golden_dir, "a")
    P, F = fx["P"], fx["F"]
    args = (fx["pts"], fx["feat"], P, F, fx["conf"], fx["desc_conf"])
    tol = head_ref.bounds(*args)
    B, S, _ = fx["feat"].shape
    # (i, j) swapped inside the patch, and the channel taken as the fastest index
    swapped = fx["feat"].reshape(B, S, F + 1, P, P).transpose(0, 1, 2, 4, 3).reshape(B, S, -1)
    chan_last = fx["feat"].reshape(B, S, P * P, F + 1).transpose(0, 1, 3, 2).reshape(B, S, -1)
    for what, feat in (("i and j swapped", swapped), ("channel fastest", chan_last)):
        wrong = head_ref.head_exact(fx["pts"], np.ascontiguousarray(feat), P, F, fx["conf"], fx["desc_conf"])
        for key in ("D", "Q"):
            err = np.abs(wrong[key] - fx[OUT[key]])
            assert float((err > tol[key]).mean()) > 0.9, (what, key)


def test_downsample_is_a_strided_view_of_the_exact_result(golden_dir):
    fx = load(golden_dir, "c")
    args = (fx["pts"], fx["feat"], fx["P"], fx["F"], fx["conf"], fx["desc_conf"])
    full = head_ref.head_exact(*args)
    for ds in (2, 3):
        sub = head_ref.head_exact(*args, ds=ds)
        for key in OUT:
            assert np.array_equal(sub[key], full[key][:, ::ds, ::ds]), (ds, key)


def test_torch_tail_agrees_in_fp32(golden_dir):
    fx = load(golden_dir, "e")
    B, _, H, W = fx["pts"].shape
    got = head_ref.head_torch(torch.from_numpy(fx["pts"]), torch.from_numpy(fx["feat"]), H, W, fx["P"], fx["F"],
                              fx["conf"], fx["desc_conf"])
    args = (fx["pts"], fx["feat"], fx["P"], fx["F"], fx["conf"], fx["desc_conf"])
    exact, tol = head_ref.head_exact(*args), head_ref.bounds(*args)
    for key, g in zip(("X", "C", "D", "Q"), got):
        ok, worst = head_ref.compare(g.numpy(), exact[key], tol[key])
        assert ok, (key, worst)


def test_special_values_of_the_exact_statement():
    P, F, H, W = 2, 3, 2, 4
    pts = np.ones((1, 4, H, W), np.float32)
    feat = np.ones((1, 2, (F + 1) * P * P), np.float32)
    pts[0, :3, 0, 0] = 0.0                 # zero point -> 0
    pts[0, 3, 0, 1], pts[0, 3, 0, 2] = 100.0, -100.0
    feat[0, 1, [0 * 4 + 3, 1 * 4 + 3, 2 * 4 + 3]] = 0.0  # token 1, (i, j) = (1, 1) -> pixel (1, 3): zero descriptor
    feat[0, 0, 3 * 4 + 0] = np.nan         # raw desc conf of pixel (0, 0)
    ex = head_ref.head_exact(pts, feat, P, F)
    assert np.array_equal(ex["X"][0, 0, 0], np.zeros(3))
    assert np.isnan(ex["D"][0, 1, 3]).all() and np.isnan(ex["D"]).sum() == F
    assert ex["C"][0, 0, 1] > float(np.finfo(np.float32).max) and abs(ex["C"][0, 0, 2] - 1.0) < 1e-40
    assert np.isnan(ex["Q"][0, 0, 0]) and np.isnan(ex["Q"]).sum() == 1
    tol = head_ref.bounds(pts, feat, P, F)
    for key in OUT:  # the statement compared with itself rounded to fp32: classes agree, error within rounding
        with np.errstate(all="ignore"):
            ok, worst = head_ref.compare(ex[key].astype(np.float32), ex[key], tol[key])
        assert ok and worst < 1.0, (key, worst)
