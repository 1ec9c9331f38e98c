"""Fixture F24: the reference's own lepard.transformer, matching, procrustes and pipeline modules on the CPU.

The reference's modules import with its `correspondence` directory on sys.path; they are run with a temporary directory OUTSIDE the
repository as the working directory (the backbone writes its kernel-point cache into ./kernels/dispositions).  Numbers only are
recorded -- inputs, state dicts (model weights are data) and outputs -- nothing of the reference's program text.  Run once where the
reference is present:

    python tests/golden/make_golden_lepard.py

Keys of tests/golden/F24_lepard.npz (tests/_lepard_ref.py names the cases):
  a.<variant>.x / source / x_pts / source_pts / lens    (a) GeometryAttentionLayer alone, C = 48, H = 4, B = 2 padded with prefix masks:
  a.<variant>.sd.<name>, a.<variant>.out / out64            inputs, the points the codes come from, state dict, float32 and double outputs
  b.<case>.src / tgt / s_pcd / t_pcd / lens              (b) RepositioningTransformer + Matching + SoftProcrustesLayer, float32, C = 24, H = 4
  b.<case>.t.sd.<name>, b.<case>.m.sd.<name>                 the transformer's and the coarse matcher's state dicts
  b.<case>.out.src / out.tgt, pl.conf / match / R / t / condition / mask, conf / match / R / t / condition
  c.sd.<name>                                            (c) Pipeline on fixture F23's batch; backbone.* is F23's c.sd.* and is not repeated
  c.conf / match / R / t, c.pl.conf / match / R / t / condition / mask
The (b) inputs are reseeded until, in the float64 restatement, every condition number is at least 10 % away from max_condition_num,
the confidence gap at every top-n cut exceeds twice the bar, and the reference's float32 numbers agree with the float64
restatement inside the bar (tests/_lepard_ref.b_preconditions; asserted here and again in tests/test_lepard_cpu.py).

float64 truth behind a positioning layer never comes from reference.double(): SoftProcrustesLayer casts R to float32, the next line
raises on the mixed types, and its bare `except` returns the identity with condition 0."""
import copy
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import _kpfcn_ref as K  # noqa: E402
from tests import _lepard_ref as P  # noqa: E402

REF = "/root/reference/correspondence"


def padded(rows_list, width):
    out = np.zeros((len(rows_list), max(r.shape[0] for r in rows_list), width), np.float32)
    for b, r in enumerate(rows_list):
        out[b, :r.shape[0]] = r
    return out


def main():
    tmp = tempfile.mkdtemp()
    assert not os.path.abspath(tmp).startswith(ROOT)
    os.chdir(tmp)
    sys.path.insert(0, REF)
    import torch
    from lepard.matching import Matching
    from lepard.pipeline import Pipeline
    from lepard.position_encoding import VolumetricPositionEncoding
    from lepard.procrustes import SoftProcrustesLayer
    from lepard.transformer import GeometryAttentionLayer, RepositioningTransformer

    torch.set_num_threads(8)
    out = {}
    T = torch.from_numpy

    def mask_of(lens, n):
        return torch.arange(n)[None, :] < torch.tensor(lens)[:, None]

    def jiggle_norms(module, g):
        """LayerNorm's default weight 1 / bias 0 would hide them: draw both."""
        for m in module.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.data = 1 + 0.2 * torch.randn(m.weight.shape, generator=g)
                m.bias.data = 0.2 * torch.randn(m.bias.shape, generator=g)

    # ------------------------------------------------------------------ (a) the layer alone
    C, H = 48, 4
    for vi, variant in enumerate(P.F24_LAYER_VARIANTS):
        torch.manual_seed(100 + vi)
        g = torch.Generator().manual_seed(200 + vi)
        pe_type = "sinusoidal" if variant == "sinusoidal" else "rotary"
        cfg = P.transformer_config(C, H, pe_type)
        layer = GeometryAttentionLayer(cfg)
        jiggle_norms(layer, g)
        lens = P.F24_LAYER_LENS
        xs = [torch.randn(l, C, generator=g).numpy() for l, _ in lens]
        ss = [torch.randn(s, C, generator=g).numpy() for _, s in lens]
        xp = [(torch.rand(l, 3, generator=g) + torch.tensor(P.VOL_BNDS[0])).numpy() for l, _ in lens]
        sp = [(torch.rand(s, 3, generator=g) + torch.tensor(P.VOL_BNDS[0])).numpy() for _, s in lens]
        x, s, xpts, spts = padded(xs, C), padded(ss, C), padded(xp, 3), padded(sp, 3)
        xm, sm = mask_of([l for l, _ in lens], x.shape[1]), mask_of([v for _, v in lens], s.shape[1])
        res = []
        for dt in (torch.float32, torch.float64):
            vol = VolumetricPositionEncoding(P.transformer_config(C, H, pe_type))
            lay = copy.deepcopy(layer).to(dt)
            with torch.no_grad():
                x_pe, s_pe = (None, None) if variant == "none" else (vol(T(xpts).to(dt)), vol(T(spts).to(dt)))
                res.append(lay(T(x).to(dt), T(s).to(dt), x_pe, s_pe, xm, sm).numpy())
        p = f"a.{variant}."
        out.update({p + "x": x, p + "source": s, p + "x_pts": xpts, p + "source_pts": spts, p + "lens": np.asarray(lens, np.int32),
                    p + "out": res[0], p + "out64": res[1]})
        out.update({p + "sd." + k: v.numpy() for k, v in layer.state_dict().items()})
        print("(a)", variant, "f32 - f64", float(np.abs(res[0] - res[1]).max()), flush=True)

    # ------------------------------------------------------------------ (b) transformer + matcher + soft-Procrustes
    C, H = 24, 4
    cfg = P.transformer_config(C, H)
    for ci, case in enumerate(P.F24_B_CASES):
        lens = P.F24_B_LENS[case]
        for seed in range(1000 * (ci + 1), 1000 * (ci + 1) + 400):
            torch.manual_seed(seed)
            g = torch.Generator().manual_seed(seed + 7)
            net, matcher, sp = RepositioningTransformer(cfg), Matching(cfg.feature_matching), SoftProcrustesLayer(cfg.procrustes)
            jiggle_norms(net, g)
            srcs = [torch.randn(s, C, generator=g).numpy() for s, _ in lens]
            tgts = [torch.randn(t, C, generator=g).numpy() for _, t in lens]
            sps = [(torch.rand(s, 3, generator=g) + torch.tensor(P.VOL_BNDS[0])).numpy() for s, _ in lens]
            tps = [(torch.rand(t, 3, generator=g) + torch.tensor(P.VOL_BNDS[0])).numpy() for _, t in lens]
            src, tgt, s_pcd, t_pcd = padded(srcs, C), padded(tgts, C), padded(sps, 3), padded(tps, 3)
            sm, tm = mask_of([s for s, _ in lens], src.shape[1]), mask_of([t for _, t in lens], tgt.shape[1])
            data = {}
            with torch.no_grad():
                fs, ft, spe, tpe = net(T(src), T(tgt), T(s_pcd), T(t_pcd), sm, tm, data)
                conf, match = matcher(fs, ft, spe, tpe, sm, tm, data, pe_type=cfg.pe_type)
                R, t, _, _, cond, _ = sp(conf, T(s_pcd), T(t_pcd), sm, tm)
            pl = data["position_layers"][1]
            p = f"b.{case}."
            rec = {p + "src": src, p + "tgt": tgt, p + "s_pcd": s_pcd, p + "t_pcd": t_pcd, p + "lens": np.asarray(lens, np.int32),
                   p + "out.src": fs.numpy(), p + "out.tgt": ft.numpy(), p + "pl.conf": pl["conf_matrix"].numpy(),
                   p + "pl.match": pl["match_pred"].numpy().astype(np.int32), p + "pl.R": pl["R_s2t_pred"].numpy(), p + "pl.t": pl["t_s2t_pred"].numpy(),
                   p + "pl.condition": pl["condition"].numpy(), p + "pl.mask": pl["solution_mask"].numpy(), p + "conf": conf.numpy(),
                   p + "match": match.numpy().astype(np.int32), p + "R": R.numpy(), p + "t": t.numpy(), p + "condition": cond.numpy()}
            rec.update({p + "t.sd." + k: v.numpy() for k, v in net.state_dict().items()})
            rec.update({p + "m.sd." + k: v.numpy() for k, v in matcher.state_dict().items()})
            ok, why = P.b_preconditions(rec, case)
            print("(b)", case, "seed", seed, "conditions", pl["condition"].numpy(), cond.numpy(), "ok" if ok else f"no: {why}", flush=True)
            if ok:
                out.update(rec)
                break
        assert ok, f"(b) {case}: no seed met the preconditions"

    # ------------------------------------------------------------------ (c) the pipeline on F23's batch
    batch, z23 = K.load_f23()
    pcfg = P.pipeline_config()
    torch.manual_seed(24)
    pipe = Pipeline(pcfg)
    jiggle_norms(pipe.coarse_transformer, torch.Generator().manual_seed(25))
    pipe.backbone.load_state_dict({k: T(np.asarray(v)) for k, v in K.state_dict(z23, "c.sd.").items()}, strict=True)
    lens = [int(v) for v in batch["stack_lengths"][pcfg.kpfcn_config.coarse_level]]
    n0, n1 = lens
    data = {"points": [T(p) for p in batch["points"]], "stack_lengths": [T(np.asarray(v)) for v in batch["stack_lengths"]],
            "features": T(batch["features"]), "src_mask": torch.ones(1, n0, dtype=torch.bool), "tgt_mask": torch.ones(1, n1, dtype=torch.bool),
            "src_ind_coarse_split": torch.arange(n0), "tgt_ind_coarse_split": torch.arange(n1), "src_ind_coarse": torch.arange(n0),
            "tgt_ind_coarse": n0 + torch.arange(n1)}
    for key in ("neighbors", "pools", "upsamples"):
        data[key] = [T(t.astype(np.int64)) for t in batch[key]]
    with torch.no_grad():
        res = pipe(data)
    pl = res["position_layers"][1]
    out.update({"c.conf": res["conf_matrix_pred"].numpy(), "c.match": res["coarse_match_pred"].numpy().astype(np.int32), "c.R": res["R_s2t_pred"].numpy(),
                "c.t": res["t_s2t_pred"].numpy(), "c.pl.conf": pl["conf_matrix"].numpy(), "c.pl.match": pl["match_pred"].numpy().astype(np.int32),
                "c.pl.R": pl["R_s2t_pred"].numpy(), "c.pl.t": pl["t_s2t_pred"].numpy(), "c.pl.condition": pl["condition"].numpy(),
                "c.pl.mask": pl["solution_mask"].numpy()})
    out.update({"c.sd." + k: v.numpy() for k, v in pipe.state_dict().items() if not k.startswith("backbone.")})
    print("(c) coarse", lens, "matches", res["coarse_match_pred"].shape[0], "condition", pl["condition"].numpy(), flush=True)

    path = os.path.join(HERE, "F24_lepard.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 900 * 1024


if __name__ == "__main__":
    main()
