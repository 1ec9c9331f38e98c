"""Fixture F25: the reference's own outlier_rejection.pipeline, geometry_attention, position_encoding and loss modules on the CPU.

The reference's modules import with its `correspondence` directory on sys.path and run with plain torch; its configs are read as
config['x'] and config.x alike, which a dict with attribute access serves.  Numbers only are recorded -- inputs, state dicts (model
weights are data) and outputs -- nothing of the reference's program text.  Run once where the reference is present:

    python tests/golden/make_golden_outlier.py

Keys of tests/golden/F25_outlier.npz (tests/_outlier_ref.py names the cases):
  a.<variant>.x / source / vec6d / lens          (a) CorrespondenceAttentionLayer alone with the compatibility of vec6d, C = 48, H = 4,
  a.<variant>.sd.<name>, a.<variant>.out / out64     B = 2 padded with prefix masks: inputs, state dict, float32 and double outputs
  b.s_pcd / t_pcd / match / sd.<name>            (b) Outlier_Rejection, 2 layers, C = 48, H = 4, two pairs of 37 and 21 matches
  b.conf / conf64 / positive_share                   the float32 and double confidences (padded), the share of c > 0 per pair
  b1.*                                           (b') the same with one layer at C = 72, H = 4: D = 18, the shipped head width
  c.flow / rot / trn / mask / rate               (c) NeCoLoss.compute_inlier_mask on (b) at inlier_thr = 0.04
The last classification layer of (b) / (b') is re-centred and scaled so that the float64 confidences spread around the threshold 0.5;
the inputs are reseeded until tests/_outlier_ref.net_preconditions and inlier_preconditions hold (asserted here and again in
tests/test_outlier_cpu.py)."""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import _outlier_ref as O  # noqa: E402

REF = "/root/reference/correspondence"


def padded(rows_list, dtype=np.float32):
    out = np.zeros((len(rows_list), max(r.shape[0] for r in rows_list)) + rows_list[0].shape[1:], dtype)
    for b, r in enumerate(rows_list):
        out[b, :r.shape[0]] = r
    return out


def pair(n, m, g):
    """n coarse points a side, m matches -> s_pcd, t_pcd, flow, rot, trn, match rows (s, t): target i is source i warped plus noise;
    about 60 % of the matches are (i, i), the others point at a random other target."""
    s = g.uniform(-0.6, 0.6, (n, 3))
    flow = 0.03 * np.sin(3.0 * s[:, ::-1])
    ax = g.standard_normal(3)
    ax /= np.linalg.norm(ax)
    ang = 0.5
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    rot = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
    trn = g.uniform(-0.3, 0.3, (3, 1))
    t = (rot @ (s + flow).T + trn).T + 0.01 * g.standard_normal((n, 3))
    si = np.sort(g.permutation(n)[:m])
    ti = si.copy()
    bad = g.uniform(0, 1, m) < 0.4
    ti[bad] = (si[bad] + g.integers(1, n, int(bad.sum()))) % n
    f = lambda a: a.astype(np.float32)
    return f(s), f(t), f(flow), f(rot), f(trn), np.stack([si, ti], 1)


def main():
    sys.path.insert(0, REF)
    import torch
    from outlier_rejection.geometry_attention import CorrespondenceAttentionLayer
    from outlier_rejection.loss import NeCoLoss
    from outlier_rejection.pipeline import Outlier_Rejection
    from outlier_rejection.position_encoding import VolumetricPositionEncoding

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
    lens = O.F25_LAYER_LENS
    for vi, variant in enumerate(O.F25_LAYER_VARIANTS):
        torch.manual_seed(300 + vi)
        g = torch.Generator().manual_seed(400 + vi)
        cfg = O.config(C, H, variant)
        layer = CorrespondenceAttentionLayer(cfg)
        jiggle_norms(layer, g)
        x = padded([torch.randn(n, C, generator=g).numpy() for n in lens])
        s = padded([torch.randn(n, C, generator=g).numpy() for n in lens])
        v6 = padded([O.matches(n, 500 + 10 * vi + b) for b, n in enumerate(lens)])
        m = mask_of(lens, x.shape[1])
        share = [float((O.compat(v6[b, :n], v6[b, :n]) > 0).mean()) for b, n in enumerate(lens)]
        assert all(0.1 <= v <= 0.9 for v in share), share
        res = []
        for dt, ndt in ((torch.float32, np.float32), (torch.float64, np.float64)):
            lay = copy.deepcopy(layer).to(dt)
            comp = T(np.stack([O.compat(v6[b], v6[b], dtype=ndt) for b in range(len(lens))]))
            with torch.no_grad():
                pe = None if variant == "none" else VolumetricPositionEncoding(cfg)(T(v6).to(dt))
                res.append(lay(T(x).to(dt), T(s).to(dt), pe, pe, m, m, compatibility=comp).numpy())
        p = f"a.{variant}."
        out.update({p + "x": x, p + "source": s, p + "vec6d": v6, p + "lens": np.asarray(lens, np.int32), p + "out": res[0], p + "out64": res[1],
                    p + "positive_share": np.asarray(share)})
        out.update({p + "sd." + k: v.numpy() for k, v in layer.state_dict().items()})
        print("(a)", variant, "f32 - f64", float(np.abs(res[0] - res[1]).max()), "positive share", share, flush=True)

    # ------------------------------------------------------------------ (b), (b') the network; (c) the inlier mask on (b)
    for ni, name in enumerate(O.F25_NETS):
        spec, cfg = O.F25_NETS[name], O.net_config(name)
        for seed in range(2000 * (ni + 1), 2000 * (ni + 1) + 400):
            torch.manual_seed(seed)
            g = torch.Generator().manual_seed(seed + 7)
            ng = np.random.default_rng(seed + 11)
            net = Outlier_Rejection(cfg)
            jiggle_norms(net, g)
            pairs = [pair(O.F25_POINTS, m, ng) for m in spec["lens"]]
            s_pcd, t_pcd = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
            match = np.concatenate([np.concatenate([np.full((len(p[5]), 1), b), p[5]], 1) for b, p in enumerate(pairs)]).astype(np.int64)
            p_ = name + "."
            rec = {p_ + "s_pcd": s_pcd, p_ + "t_pcd": t_pcd, p_ + "match": match.astype(np.int32)}
            v6 = O.net_vec6d(rec, name)
            rec[p_ + "positive_share"] = np.asarray([float((O.compat(v, v) > 0).mean()) for v in v6])
            # re-centre and scale the last layer on the float64 logits of the restatement
            sd = {k: v.numpy() for k, v in net.state_dict().items()}
            z = np.concatenate([O.network(sd, cfg, v, np.float64)[0] for v in v6])
            gain = 3.0 / float(z.std())
            last = net.classification[4]
            last.bias.data = ((last.bias.data.double() - float(np.median(z))) * gain).float()
            last.weight.data = (last.weight.data.double() * gain).float()
            rec.update({p_ + "sd." + k: v.numpy() for k, v in net.state_dict().items()})
            res = []
            for dt in (torch.float32, torch.float64):
                data = {"s_pcd": T(s_pcd).to(dt), "t_pcd": T(t_pcd).to(dt), "coarse_match_pred": T(match)}
                with torch.no_grad():
                    res.append((copy.deepcopy(net).to(dt).eval()(data).numpy(), data))
            rec.update({p_ + "conf": res[0][0], p_ + "conf64": res[1][0]})
            ok, why = O.net_preconditions(rec, name)
            if ok and name == "b":
                flow, rot, trn = (np.stack([p[k] for p in pairs]) for k in (2, 3, 4))
                data = res[0][1]
                data.update({"batched_rot": T(rot), "batched_trn": T(trn)})
                masks, rates = NeCoLoss.compute_inlier_mask(data, O.F25_INLIER_THR, s2t_flow=T(flow))
                rec.update({"c.flow": flow, "c.rot": rot, "c.trn": trn, "c.mask": padded([m.numpy()[:, None] for m in masks], bool)[:, :, 0],
                            "c.rate": np.asarray([float(r) for r in rates], np.float32)})
                ok, why = O.inlier_preconditions(rec)
            print(f"({name}) seed", seed, "positive share", rec[p_ + "positive_share"], "ok" if ok else f"no: {why}", flush=True)
            if ok:
                out.update(rec)
                break
        assert ok, f"({name}): no seed met the preconditions"

    path = os.path.join(HERE, "F25_outlier.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 900 * 1024


if __name__ == "__main__":
    main()
