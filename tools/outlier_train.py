"""Train the outlier rejection network on synthetic matches and save a checkpoint in the reference's layout:
    python tools/outlier_train.py --steps 200 --out neco.pth [--matches 256] [--outlier-ratio 0.4] [--lr 1e-3] [--pairs 2] [--seed 0]
Every step draws `--pairs` fresh pairs of outlier.synthetic_matches (seeds seed + 1, seed + 2, ...) and takes one Adam step of
outlier.train_step: the HIP attention forward with statistics and its backward (ops.attention_fn) under the class-weighted BCE of
the reference's NeCoLoss.  Before and after, the loss and the precision and recall of `confidence > 0.5` on one held-out batch
(four pairs with seeds counted down from 2^32 - 1, never trained on) are printed.  The file holds {'state_dict': ...} with the reference's parameter names, so
outlier.LandmarkModel.from_checkpoints and eval_supervised.py --outlier-weights load it strictly; the tool reloads the file that way
before it says so.  profiles/outlier_train.txt is this tool's standard output at --steps 200.  This is training on the
synthetic surface pairs only: 4DMatch is not available here, and nothing is claimed about the reference's own checkpoint."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deformationpyramid_amd import outlier  # noqa: E402


def batch(n, ratio, seeds, dev):
    n_out = int(round(n * ratio))
    parts = [outlier.synthetic_matches(n - n_out, n_out, s, dev) for s in seeds]
    return torch.cat([p[0] for p in parts]), [n] * len(parts), torch.cat([p[1] for p in parts])


def evaluate(model, vec_6d, lens, labels):
    conf = model.confidence(vec_6d, lens)
    loss = float(outlier.NeCoLoss.get_weighted_bce_loss(conf, labels.float()))
    kept = conf > 0.5
    tp = int((kept & labels).sum())
    return loss, tp / max(int(kept.sum()), 1), tp / max(int(labels.sum()), 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--matches", type=int, default=256, help="matches of a pair")
    ap.add_argument("--outlier-ratio", type=float, default=0.4)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--pairs", type=int, default=2, help="pairs of a step's batch")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print(f"tools/outlier_train.py, {torch.cuda.get_device_name(0)}: {a.steps} steps of Adam (lr {a.lr:g}) on {a.pairs} pairs x {a.matches} "
          f"synthetic matches a step, outlier ratio {a.outlier_ratio:g}, seed {a.seed}", flush=True)
    torch.manual_seed(a.seed)
    model = outlier.Outlier_Rejection(outlier.DEFAULT_CONFIG).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=a.lr)
    held = batch(a.matches, a.outlier_ratio, [2 ** 32 - 1 - a.seed - i for i in range(4)], dev)  # seeds that training never draws
    print("held-out batch before: loss %.5f  precision %.3f  recall %.3f" % evaluate(model, *held), flush=True)
    for step in range(a.steps):
        v6, lens, labels = batch(a.matches, a.outlier_ratio, [a.seed + 1 + step * a.pairs + i for i in range(a.pairs)], dev)
        loss = outlier.train_step(model, opt, v6, lens, labels)
        if step % max(a.steps // 10, 1) == 0 or step == a.steps - 1:
            print(f"step {step:5d}  loss {float(loss):.5f}", flush=True)
    print("held-out batch after:  loss %.5f  precision %.3f  recall %.3f" % evaluate(model, *held), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    torch.save({"state_dict": {k: v.cpu() for k, v in model.state_dict().items()}}, a.out)
    strict = outlier.Outlier_Rejection(outlier.DEFAULT_CONFIG)
    strict.load_state_dict(torch.load(a.out, map_location="cpu")["state_dict"], strict=True)
    print("saved", a.out, "-- it loads with load_state_dict(strict=True), the call LandmarkModel.from_checkpoints makes for the filter")


if __name__ == "__main__":
    main()
