#!/usr/bin/env python3
"""Device time of the warp Jacobian and the inverse warp next to what existed before them.

    python tools/jacobian_timing.py [--reps 60] [--out profiles/jacobian_inverse_timing.txt]
    python tools/jacobian_timing.py --once            (each variant a few times, no timing: the workload for rocprofv3 --kernel-trace)

Seeded m = 9 pyramids (generator seed 11, heads x 30, k0 = -8) at 128 / 3 (the MFMA kernels) and 64 / 2 (the generic ones), n = 8192 and
n = 24 856 points (the shape-transfer vertex count).  Four variants, alternated inside one process, device events around each call,
median over `reps` warmed repetitions:
  (a) ops.pyramid_fwd, fp32                      (one launch)
  (b) Deformation_Pyramid.warp_jacobian          (one launch: x' and J)
  (c) J by three autograd passes through warp()  (the only route before: m level forwards + 3 x 2 m backward launches, from Python)
  (d) Deformation_Pyramid.inverse_warp(y = W(x), iters = 8)   (one launch: every Newton pass inside)
Reported beside them: (b) / (a) next to the four-plane work ratio 4, and (d) / (b) next to the Newton passes actually run (the largest
iteration count of any point + 1 evaluations).
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deformationpyramid_amd import ops                               # noqa: E402
from deformationpyramid_amd.nets import Deformation_Pyramid          # noqa: E402

SHAPES = {"128/3": dict(width=128, depth=3), "64/2": dict(width=64, depth=2)}
SIZES = (8192, 24856)


def pyramid(shape, dev, m=9, k0=-8, scale=30.0):
    torch.manual_seed(11)
    pyr = Deformation_Pyramid(device=dev, k0=k0, m=m, rotation_format="axis_angle", motion="SE3", **SHAPES[shape])
    with torch.no_grad():
        for lvl, d in enumerate(pyr.descs):
            pyr.store[lvl, d.off_Wh:d.param_count] *= scale
    pyr.gradient_setup(optimized_level=-1)
    return pyr


def autograd_jacobian(pyr, x):
    xx = x.clone().requires_grad_(True)
    y, _ = pyr.warp(xx)
    return torch.stack([torch.autograd.grad(y[:, a].sum(), xx, retain_graph=a < 2)[0] for a in range(3)], dim=1)


def variants(pyr, x, y):
    d, m = pyr.descs[-1], pyr.n_hierarchy
    return {
        "a pyramid_fwd": lambda: ops.pyramid_fwd(d, m, pyr.k0, pyr.store, x),
        "b warp_jacobian": lambda: pyr.warp_jacobian(x),
        "c autograd x3": lambda: autograd_jacobian(pyr, x),
        "d inverse_warp": lambda: pyr.inverse_warp(y, iters=8),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU timing of these kernels"
    dev = torch.device("cuda:0")
    lines = [f"device: {torch.cuda.get_device_name(0)}; median of {args.reps} repetitions after {args.warmup} warm-ups, variants alternated, "
             "device events; ms per call", ""]
    for shape in SHAPES:
        pyr = pyramid(shape, dev)
        for n in SIZES:
            g = torch.Generator().manual_seed(41)
            x = (torch.rand(n, 3, generator=g) - 0.5).to(dev)
            y = ops.pyramid_fwd(pyr.descs[-1], pyr.n_hierarchy, pyr.k0, pyr.store, x)
            fns = variants(pyr, x, y)
            J = fns["b warp_jacobian"]()[1]
            Ja = fns["c autograd x3"]()
            diff = (J - Ja).abs().max().item() / Ja.abs().max().item()
            xs, info = fns["d inverse_warp"]()
            passes = int(info.iterations.max().item()) + 1
            if args.once:
                for _ in range(3):
                    for f in fns.values():
                        f()
                torch.cuda.synchronize()
                continue
            for _ in range(args.warmup):
                for f in fns.values():
                    f()
            torch.cuda.synchronize()
            ms = {k: [] for k in fns}
            for _ in range(args.reps):
                for k, f in fns.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f()
                    e1.record()
                    e1.synchronize()
                    ms[k].append(e0.elapsed_time(e1))
            med = {k: statistics.median(v) for k, v in ms.items()}
            lines.append(f"{shape}  m = 9  n = {n}:   J (kernel) against J (autograd): max rel diff {diff:.2e};  inverse: "
                         f"{int(info.converged.sum())}/{n} converged, max |x - known| {(xs - x).abs().max().item():.2e}")
            for k in fns:
                v = sorted(ms[k])
                lines.append(f"    ({k[0]}) {k[2:]:16s} {med[k]:9.4f} ms   (p10 {v[len(v) // 10]:.4f}, p90 {v[len(v) * 9 // 10]:.4f})")
            a, b, c, dd = (med[k] for k in fns)
            lines.append(f"    (b) < (c): {b < c}   (c) / (b) = {c / b:.1f}   (b) / (a) = {b / a:.2f} (four-plane work ratio: 4)   "
                         f"(d) / (b) = {dd / b:.2f} (Newton evaluations run: {passes})")
            lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
