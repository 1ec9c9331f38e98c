"""Fixture F23: the reference's own lepard.blocks and lepard.backbone.KPFCN on the CPU, on the (700, 500) surface pair of fixture F22.

The reference's modules import with its `correspondence` directory on sys.path; they are run with a temporary directory OUTSIDE the
repository as the working directory, because the reference writes its kernel-point cache into ./kernels/dispositions.  Numbers only
are recorded -- inputs, state dicts (model weights are data) and outputs -- nothing of the reference's program text.  Run once where
the reference is present:

    python tests/golden/make_golden_kpfcn.py

The batch: F22's level-0 points, the tables of tests/_kpconv_ref.build_pyramid with PYRAMID_LIMITS (stored as int16), ones as
features.  The config is configs/lepard.yaml's kpfcn_config with first_feats_dim 16, coarse_feature_dim 12, fine_feature_dim 8
(tests/_kpfcn_ref.F23_CONFIG).  Keys of tests/golden/F23_kpfcn.npz:
  levels, l<l>.points / lengths / neighbors / pools / upsamples      the collate's lists, 4 levels
  x8, x16                                                            float16 [1200, 8 / 16]: the input features of (a) and (b)
  a<i>.weights, a<i>.kernel_points, a<i>.out                         three bare KPConv calls (_kpfcn_ref.F23_CONVS), 8 -> 8 channels on x8
  b<i>.sd.<name>, b<i>.out                                           the three blocks (_kpfcn_ref.F23_BLOCKS) on x8 / x16, with their state dicts
  c.sd.<name>, c.out, c.out64                                        KPFCN's state dict and its coarse forward
out is the reference in float32, c.out64 the same network in double on the same float32 inputs.  The weights are reseeded
(torch.manual_seed and np.random.seed) until every KPConv input row of the blocks and of the network clears 2^-12 of its
absolute sum and has the same positive-row flag in both precisions (asserted below)."""
import copy
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import _kpconv_ref as R  # noqa: E402
from tests import _kpfcn_ref as K  # noqa: E402

REF = "/root/reference/correspondence"


def main():
    tmp = tempfile.mkdtemp()
    assert not os.path.abspath(tmp).startswith(ROOT)
    os.chdir(tmp)
    sys.path.insert(0, REF)
    import torch
    from lepard import blocks as B
    from lepard.backbone import KPFCN

    torch.set_num_threads(8)
    cfg = SimpleNamespace(**K.F23_CONFIG)
    f22 = np.load(os.path.join(HERE, "F22_kpconv.npz"))
    pts, lengths = f22["l0.points"], f22["l0.lengths"]
    pyr = R.build_pyramid(pts, lengths, architecture=R.KPFCN, limits=R.PYRAMID_LIMITS, **R.LEPARD)
    levels = len(pyr.points)
    out = {"levels": np.int32(levels)}
    for l in range(levels):
        out[f"l{l}.points"], out[f"l{l}.lengths"] = pyr.points[l], np.asarray(pyr.stack_lengths[l], np.int32)
        for key in ("neighbors", "pools", "upsamples"):
            tab = getattr(pyr, key)[l]
            assert tab.max(initial=0) < 32768
            out[f"l{l}.{key}"] = tab.astype(np.int16)

    def batch_of(dtype):
        b = {"points": [torch.from_numpy(p).to(dtype) for p in pyr.points], "stack_lengths": [torch.from_numpy(np.asarray(v)) for v in pyr.stack_lengths],
             "features": torch.ones(pts.shape[0], 1, dtype=dtype)}
        for key in ("neighbors", "pools", "upsamples"):
            b[key] = [torch.from_numpy(t.astype(np.int64)) for t in getattr(pyr, key)]
        return b

    b32, b64 = batch_of(torch.float32), batch_of(torch.float64)
    r0 = cfg.first_subsampling_dl * cfg.conv_radius

    def watched(module, call):
        """call(module) with every KPConv's input features recorded -> (output, [features])."""
        seen, hooks = [], []
        for m in module.modules():
            if isinstance(m, B.KPConv):
                hooks.append(m.register_forward_pre_hook(lambda mod, args: seen.append(args[3].detach().numpy().copy())))
        with torch.no_grad():
            y = call(module)
        for h in hooks:
            h.remove()
        return y.numpy(), seen

    def both(module, call32, call64):
        y32, in32 = watched(module, call32)
        y64, in64 = watched(copy.deepcopy(module).double(), call64)
        ok = all(K.row_clearance(a.astype(np.float64)) >= K.ROW_CLEARANCE and K.row_clearance(a) >= K.ROW_CLEARANCE
                 and np.array_equal(a.sum(1) > 0, b.sum(1) > 0) for a, b in zip(in32, in64))
        return y32, y64, ok

    for seed in range(64):
        torch.manual_seed(seed)
        np.random.seed(seed)
        xs = {c: torch.randn(pts.shape[0], c).half() for c in (8, 16)}          # float16 values: stored in half the bytes, exact in float32
        rec, good = {f"x{c}": v.numpy() for c, v in xs.items()}, True
        for i, (influence, aggregation, strided) in enumerate(K.F23_CONVS):
            conv = B.KPConv(cfg.num_kernel_points, 3, 8, 8, r0 * cfg.KP_extent / cfg.conv_radius, r0, fixed_kernel_points="center",
                            KP_influence=influence, aggregation_mode=aggregation)
            x = xs[8].float()
            tabs = lambda b: (b["points"][1], b["points"][0], b["pools"][0]) if strided else (b["points"][0], b["points"][0], b["neighbors"][0])
            y32, _, _ = both(conv, lambda m: m(*tabs(b32), x), lambda m: m(*tabs(b64), x.double()))
            rec.update({f"a{i}.weights": conv.weights.detach().numpy(), f"a{i}.kernel_points": conv.kernel_points.detach().numpy(), f"a{i}.out": y32})
        for i, (name, cin, cout) in enumerate(K.F23_BLOCKS):
            block = B.block_decider(name, r0, cin, cout, 0, cfg)
            x = xs[cin].float()
            y32, _, ok = both(block, lambda m: m(x, b32), lambda m: m(x.double(), b64))
            good &= ok
            rec[f"b{i}.out"] = y32
            rec.update({f"b{i}.sd.{k}": v.numpy() for k, v in block.state_dict().items()})
        net = KPFCN(cfg)
        y32, y64, ok = both(net, lambda m: m(b32, phase="coarse"), lambda m: m(b64, phase="coarse"))
        good &= ok
        rec.update({"c.out": y32, "c.out64": y64})
        rec.update({f"c.sd.{k}": v.numpy() for k, v in net.state_dict().items()})
        print("seed", seed, "clear" if good else "not clear", "| coarse", y32.shape, "f32 - f64", float(np.abs(y32 - y64).max()),
              "magnitude", float(np.abs(y64).max()), flush=True)
        if good:
            break
    assert good, "no seed met the clearance"
    out.update(rec)
    path = os.path.join(HERE, "F23_kpfcn.npz")
    np.savez_compressed(path, **out)
    n_par = sum(int(np.prod(v.shape)) for k, v in out.items() if k.startswith("c.sd."))
    print("levels", [p.shape[0] for p in pyr.points], "parameters", n_par, "output", y32.shape, "seed", seed, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 900 * 1024


if __name__ == "__main__":
    main()
