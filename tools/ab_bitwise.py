"""Bitwise A/B of two library builds on the same solves (GPU box).

  python tools/ab_bitwise.py variants/lib_OLD.so            # vs the in-tree library
  python tools/ab_bitwise.py variants/lib_OLD_test.so TREE  # vs another build, e.g. the tree's test library

Each library runs in its own process (M3S_LIB) on identical seeded graphs, one
or more per solve path (be.plan_path, printed per case): C3-shaped calib (32
KFs) and a small rays graph (lds_plan), 63 KFs (lds), the chip-wide path with
and without a dense tail (140, 256 KFs), the complete graph on 201 KFs (dense)
and, on test libraries (the knobs of a case are set where the loaded library
knows them), 140 KFs on the one-workgroup kernel (global_split, global); a few
GN iterations each; poses, dx and info are compared bit for bit and the solve
time of each is printed (HIP events, median)."""
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# (key, mode, N, H, W, iterations, knobs)
CASES = [("calib_32", "calib", 32, 128, 128, 10, {"dense_tail_min": 16}),
         ("rays_12", "rays", 12, 48, 64, 5, {"dense_tail_min": 16}),
         ("rays_63", "rays", 63, 24, 32, 3, {"dense_tail_min": 16}),
         ("rays_140", "rays", 140, 24, 32, 3, {"dense_tail_min": 8}),
         ("rays_140_notail", "rays", 140, 24, 32, 3, {"dense_tail_min": 0}),
         ("rays_256", "rays", 256, 12, 16, 3, {"dense_tail_min": 16}),
         ("rays_201_complete", "rays", 201, 8, 12, 2, {}),
         ("rays_140_cols0", "rays", 140, 24, 32, 3, {"dense_tail_min": 8, "cols": 0}),
         ("rays_140_cols0_nosplit", "rays", 140, 24, 32, 3, {"dense_tail_min": 8, "cols": 0, "border_split": 0})]


def child(out_path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam-ysh_amd")]
    import numpy as np
    import torch

    import mast3r_slam_backends as be
    from mast3r_slam_amd import synthetic

    dev = torch.device("cuda:0")
    res = {}
    for key, mode, N, H, W, iters, knobs in CASES:
        old = {}
        for name, value in knobs.items():
            try:
                old[name] = be.set_knob(name, value)
            except RuntimeError:  # a test-only knob on a product library
                pass
        edges = ([i for j in range(N) for i in range(j)], [j for j in range(N) for i in range(j)])
        g = synthetic.make_graph(N, H, W, seed=4242 + N, device=dev, edges=edges if "complete" in key else None)
        ranks = np.unique(torch.cat([g.ii, g.jj]).cpu().numpy(), return_inverse=True)[1].reshape(2, -1)
        res[key + "_path"] = np.array(be.plan_path(N, H * W, *ranks))
        Xs = (g.Xs[..., 2:3] * synthetic.pixel_rays(H, W, g.K)[None]).contiguous() if mode == "calib" else g.Xs
        times = []
        for rep in range(5):
            Twc = g.T_init.data.clone().contiguous()
            info = torch.zeros(8, dtype=torch.int32, device=dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if mode == "calib":
                (dx,) = be.gauss_newton_calib(Twc, Xs, g.Cs, g.K, g.ii, g.jj, g.idx_ii2jj, g.valid_match, g.Q, H, W,
                                              -10, 1e-6, 1.0, 10.0, 0.0, 1.5, iters, 0.0, info=info)
            else:
                (dx,) = be.gauss_newton_rays(Twc, Xs, g.Cs, g.ii, g.jj, g.idx_ii2jj, g.valid_match, g.Q, 0.003,
                                             10.0, 0.0, 1.5, iters, 0.0, info=info)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        for name, value in old.items():
            be.set_knob(name, value)
        res[key + "_T"] = Twc.cpu().numpy()
        res[key + "_dx"] = dx.cpu().numpy()
        res[key + "_info"] = info.cpu().numpy()
        res[key + "_ms"] = np.array(sorted(times)[2])
    np.savez(out_path, **res)


def main():
    import numpy as np

    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(sys.argv[2])
        return
    variant = os.path.abspath(sys.argv[1])
    tree = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else None
    outs = []
    for tag, lib in (("tree", tree), ("variant", variant)):
        env = dict(os.environ)
        if lib:
            env["M3S_LIB"] = lib
        path = os.path.join(ROOT, "gpurun_out", f"ab_{tag}.npz")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        subprocess.run([sys.executable, __file__, "--child", path], check=True, env=env, timeout=600)
        outs.append(np.load(path))
    a, b = outs
    ok = True
    for key, *_ in CASES:
        same = all(np.array_equal(a[key + s], b[key + s]) for s in ("_T", "_dx", "_info", "_path"))
        ok &= same
        print(f"{key:24s} {str(a[key + '_path']):12s} bitwise {'EQUAL' if same else 'DIFFERENT'}  max|dT| {np.abs(a[key + '_T'] - b[key + '_T']).max():.3e}"
              f"  call ms: tree {float(a[key + '_ms']):.4f} variant {float(b[key + '_ms']):.4f}  "
              f"fails {a[key + '_info'][1]}/{b[key + '_info'][1]}")
    print("ALL EQUAL" if ok else "SOME DIFFERENT")


if __name__ == "__main__":
    main()
