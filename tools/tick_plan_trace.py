#!/usr/bin/env python3
"""The launches of the engine's tick under a kernel trace, to compare two builds dispatch by dispatch.

    rocprofv3 --kernel-trace -f csv -d OUT -o NAME -- python tools/tick_plan_trace.py run     # on the GPU, once per build
    python tools/tick_plan_trace.py compare OLD_kernel_trace.csv NEW_kernel_trace.csv [--labels A B] [--out FILE]

`run` builds one small engine for every branch of the tick's launch plan (the rows of tests/test_tick_plan_cpu.py, with real buffers
and a pair in every slot) and runs two ticks of each.  It uses nothing newer than BatchedEngine's constructor, load and run_ticks, so
the same file drives an older tree (put that tree first on PYTHONPATH).  `compare` lists the engine's dispatches of both traces in
dispatch order -- kernel name, grid, workgroup size, LDS block size -- and says whether they are equal line for line.
"""
import argparse
import csv
import sys

M, ITERS, TICKS = 1, 2, 2
# (gemm_mode, nn_mode, G, B, n_cap = t_cap, extras)
ENGINES = [
    (7, 2, 1, 4, 512, {}), (7 | 1024, 2, 1, 4, 512, {}),                                        # row 1
    (7, 2, 8, 4, 512, {}), (7, 2, 4, 4, 512, {}), (7, 2, 8, 64, 512, {}),                       # row 2
    (7 | 16, 2, 2, 4, 512, {}),                                                                 # row 3
    (5, 2, 2, 4, 512, {}), (5, 2, 1, 4, 512, {}),                                               # row 4
    (0, 0, 2, 4, 512, {}),                                                                      # row 5
    (7, 1, 1, 2, 512, {}), (7, 1, 1, 3, 512, {}),                                               # row 6
    (7, 2, 1, 4, 512, dict(nn_cells=True)), (7, 2, 1, 4, 4096, dict(nn_cells_wide=True)),       # row 7
    (7, 2, 2, 4, 512, dict(width=64)),                                                          # row 8
    (7, 2, 1, 4, 512, dict(w_cd=0.0)),                                                          # row 9
]


def run():
    import torch
    from deformationpyramid_amd.engine import BatchedEngine, OptConfig
    from deformationpyramid_amd.layout import LayerDesc
    dev = torch.device("cuda")
    for gemm_mode, nn_mode, G, B, cap, extra in ENGINES:
        extra = dict(extra)
        desc = LayerDesc(width=extra.pop("width", 128))
        w_cd = extra.pop("w_cd", 1.0)
        cfg = OptConfig(m=M, iters=ITERS, early_stop=False, w_cd=w_cd, trunc=1e9)
        extra.setdefault("nn_cells", False)
        extra.setdefault("nn_cells_wide", False)
        eng = BatchedEngine(desc, cfg, B, n_cap=cap, t_cap=cap, device=dev, G=G, nn_mode=nn_mode, gemm_mode=gemm_mode, **extra)
        K = 0 if w_cd else 16                          # without a Chamfer term the loss is the landmarks'
        S, T = cap - 3 - K, cap - 5
        g = torch.Generator().manual_seed(1)
        params = 0.05 * torch.randn(M, eng.p_stride, generator=g)
        for b in range(B):
            pts = torch.rand(K + S, 3, generator=g) - 0.5
            tgt = torch.rand(T, 3, generator=g) - 0.48
            eng.load(b, pts, K, S, pts[:K] + 0.01 if K else None, tgt, params)
        eng.run_ticks(TICKS)
        torch.cuda.synchronize()
        print(f"gemm_mode {gemm_mode} nn_mode {nn_mode} G {G} B {B} cap {cap} {extra} w_cd {w_cd} width {desc.width}: "
              f"{[s.total_evals for s in eng.read_states()]} evaluations", flush=True)


def dispatches(path):
    """[(kernel, grid, workgroup, lds)] of the engine's tick kernels (k_eng_*, the slot load included) in dispatch order."""
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    out = []
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].removesuffix(".kd")
        if name.startswith("k_eng_"):
            out.append((name, "x".join(r[f"Grid_Size_{a}"] for a in "XYZ"), "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ"),
                        r.get("LDS_Block_Size") or r["Group_Segment_Size"]))
    return out


def compare(args):
    la, lb = args.labels or (args.old, args.new)
    a, b = dispatches(args.old), dispatches(args.new)
    bad = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
    same = not bad and len(a) == len(b)
    lines = ["# engine tick launches under rocprofv3 --kernel-trace (tools/tick_plan_trace.py): the engines of tests/test_tick_plan_cpu.py's rows 1-9,",
             f"# iters = {ITERS}, {TICKS} ticks each; per dispatch, in dispatch order: kernel, grid (work-items), workgroup, LDS block size (bytes)",
             "# (LDS_Block_Size as the trace gives it: where it reads 0 for a kernel whose LDS is all dynamic, the trace carries the static",
             "#  size only and says nothing about the launch's dynamic bytes -- those are held by tests/test_tick_plan_cpu.py's literals)",
             f"old: {la}: {len(a)} dispatches", f"new: {lb}: {len(b)} dispatches",
             "verdict: " + ("EQUAL line for line" if same else f"DIFFERENT ({len(bad)} lines differ, lengths {len(a)} / {len(b)})"), ""]
    for tag, rows in (("old", a), ("new", b)):
        lines.append(f"## {tag}")
        lines += [f"{i:4d} {n:22s} grid {g:16s} wg {w:10s} lds {l}" + ("   <-- differs" if i in bad else "") for i, (n, g, w, l) in enumerate(rows)]
        lines.append("")
    report = "\n".join(lines)
    print("\n".join(lines[:8]))
    if args.out:
        with open(args.out, "w") as f:
            f.write(report)
    return 0 if same else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("run")
    c = sub.add_parser("compare")
    c.add_argument("old")
    c.add_argument("new")
    c.add_argument("--labels", nargs=2, default=None)
    c.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.exit(run() if args.cmd == "run" else compare(args))
