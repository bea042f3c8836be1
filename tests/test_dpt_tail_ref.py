"""CPU checks of tests/dpt_tail_ref.py against the reference's own output
(tests/golden/dpt_tail_{a..e}.npz, written by make_dpt_tail_golden.py from the
reference's Interpolate class and torch's Conv2d / ReLU in fp32): every fixture
lies within `bound` of `dpt_tail_exact`, so the header's function, with its
fp32 lambdas, is the reference's.

Fractions reached when the fixtures were written (max |reference - exact| /
bound): a 1.2e-4, b 1.2e-4, c 1.5e-4, d 9.9e-5, e 2.6e-4. The bound is a
worst-case one over 1153- and 129-term sums; an fp32 evaluation's rounding
errors largely cancel."""
import pytest
import torch

import dpt_tail_ref as ref


@pytest.fixture(scope="module")
def cases(golden_dir):
    return {n: ref.load_fixture(golden_dir, n) for n in ref.FIXTURES}


def test_fixture_shapes(cases):
    want = {"a": (2, 5, 7, 4), "b": (1, 1, 1, 4), "c": (1, 1, 5, 4), "d": (1, 3, 2, 3), "e": (1, 12, 9, 4)}
    for n, (B, Hi, Wi, cout) in want.items():
        c = cases[n]
        assert tuple(c["x"].shape) == (B, 128, Hi, Wi) and c["cout"] == cout
        assert tuple(c["out"].shape) == (B, cout, 2 * Hi, 2 * Wi) and c["out"].dtype == torch.float32
    x = cases["e"]["x"].abs()
    assert float(x.max() / x[x > 0].min()) > 1e6  # spread over several decades


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_reference_within_bound_of_exact(cases, name):
    c = cases[name]
    frac = ref.fraction(c["out"], c["x"], *c["w"])
    print(f"dpt_tail_{name}: max |reference - exact| / bound = {frac:.3g}")
    assert frac <= 1.0
    assert bool((ref.bound(c["x"], *c["w"]) > 0).all())


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_own_torch_statement_within_bound(cases, name):
    """dpt_tail_torch (the timing tool's yardstick path) and the op-by-op fp32 upsampling
    followed by torch's convolutions both compute the header's function."""
    c = cases[name]
    w1, b1, w2, b2 = c["w"]
    assert ref.fraction(ref.dpt_tail_torch(c["x"], *c["w"]), c["x"], *c["w"]) <= 1.0
    u = ref.upsample_f32(c["x"])
    out = torch.nn.functional.conv2d(torch.relu(torch.nn.functional.conv2d(u, w1, b1, padding=1)), w2, b2)
    assert ref.fraction(out, c["x"], *c["w"]) <= 1.0


def test_mid_has_many_negatives_and_large_values(cases):
    c = cases["e"]
    w1, b1, _, _ = c["w"]
    pre = torch.nn.functional.conv2d(ref.upsample_exact(c["x"]), w1.double(), b1.double(), padding=1)
    assert 0.3 < float((pre < 0).double().mean()) < 0.7
    assert float(pre.max()) > 1e3


def test_upsample_f32_against_torch_interpolate(cases):
    """Reported, nothing rests on it: whether torch-CPU F.interpolate equals the
    header's u bitwise (it evaluates the same lambdas in another order). What is
    asserted is only that the two agree to the 7 roundings of the bound."""
    for name in ref.FIXTURES:
        x = cases[name]["x"]
        u = ref.upsample_f32(x)
        t = torch.nn.functional.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        print(f"dpt_tail_{name}: F.interpolate == header's u bitwise: {torch.equal(u, t)}, "
              f"max |diff| = {float((u - t).abs().max()):.3g}")
        U = ref.upsample_exact(x, absolute=True)
        assert bool(((u.double() - t.double()).abs() <= 2 * 7 * ref.EPS32 * 1.01 * U).all())
        assert bool(((u.double() - ref.upsample_exact(x)).abs() <= 7 * ref.EPS32 * 1.01 * U).all())


def test_lambdas_are_the_headers():
    for n in (1, 2, 3, 5, 7, 9, 12, 33, 192, 256):
        i0, i1, l0, l1 = ref.lambdas(n)
        assert i0.shape == (2 * n,) and int(i0[0]) == 0 and int(i1[-1]) == n - 1
        assert bool((i0[1:] >= i0[:-1]).all()) and bool(((i1 - i0) >= 0).all()) and bool(((i1 - i0) <= 1).all())
        assert bool((l1 >= 0).all()) and bool((l1 < 1).all()) and l0.dtype == torch.float32
        # a workgroup's source tile: the rows under tile + 2 outputs (m3s_dpt.hip kSrcH, kSrcW)
        for tile, src in ((8, 7), (32, 19)):
            for a in range(0, 2 * n, tile):
                lo, hi = max(a - 1, 0), min(a + tile, 2 * n - 1)
                assert int(i1[hi]) - int(i0[lo]) + 1 <= src
