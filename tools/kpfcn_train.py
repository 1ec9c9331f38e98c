"""Train the KPFCN coarse descriptors on synthetic surface pairs through the HIP KPConv backward (kpfcn.train_step):
    python tools/kpfcn_train.py --steps 200 --out ckpt.pth [--log profiles/kpfcn_train.txt]
Prints the descriptor loss and the mutual-NN match recall on held-out pairs before and after, saves the state dict and reloads it
into a fresh kpfcn.KPFCN with strict=True.  The numbers are reported, not asserted; the tool only has to show a decrease.
profiles/kpfcn_train.txt is its output at --steps 200."""
import argparse, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deformationpyramid_amd import kpfcn
from tests import _kpfcn_ref as K

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--out", default="kpfcn_ckpt.pth")
ap.add_argument("--log", default=None)
ap.add_argument("--points", type=int, default=2048)
ap.add_argument("--pairs", type=int, default=8, help="training pairs, visited in turn")
ap.add_argument("--lr", type=float, default=1e-3)
args = ap.parse_args()
dev = torch.device("cuda:0")
cfg = {**K.F23_CONFIG, "first_subsampling_dl": 0.02, "first_feats_dim": 32, "coarse_feature_dim": 32}
lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


@torch.no_grad()
def evaluate(model, batches):
    feats = [model(b, phase="coarse") for b in batches]
    loss = sum(float(kpfcn.descriptor_loss(f, b)) for f, b in zip(feats, batches)) / len(batches)
    recall = sum(kpfcn.match_recall(f, b) for f, b in zip(feats, batches)) / len(batches)
    return loss, recall


torch.manual_seed(219)
model = kpfcn.KPFCN(cfg).to(dev)
params = kpfcn.trainable_parameters(model)
train = [kpfcn.synthetic_batch(100 + i, cfg, n_points=args.points, device=dev) for i in range(args.pairs)]
held = [kpfcn.synthetic_batch(900 + i, cfg, n_points=args.points, device=dev) for i in range(4)]
say(f"tools/kpfcn_train.py on {torch.cuda.get_device_name(0)}: KPFCN first_feats_dim {cfg['first_feats_dim']}, coarse_feature_dim "
    f"{cfg['coarse_feature_dim']}, {sum(p.numel() for p in params)} trained parameters; {args.pairs} training pairs and 4 held-out pairs of "
    f"2 x {args.points} points, coarse level {[b['coarse_lengths'] for b in held]}, matches {[int(b['matches'].shape[1]) for b in held]}; "
    f"Adam lr {args.lr}, one pair a step")
loss0, recall0 = evaluate(model, held)
say(f"held-out before: descriptor loss {loss0:.4f}   mutual-NN match recall {recall0:.3f}")
opt = torch.optim.Adam(params, lr=args.lr)
t0 = time.time()
for step in range(args.steps):
    loss = float(kpfcn.train_step(model, [train[step % len(train)]], opt))
    if step % max(1, args.steps // 10) == 0 or step == args.steps - 1:
        say(f"step {step:4d}: training loss {loss:.4f}")
torch.cuda.synchronize()
say(f"{args.steps} steps in {time.time() - t0:.1f} s")
loss1, recall1 = evaluate(model, held)
say(f"held-out after:  descriptor loss {loss1:.4f}   mutual-NN match recall {recall1:.3f}   "
    f"({'the loss decreased' if loss1 < loss0 else 'THE LOSS DID NOT DECREASE'})")
torch.save(model.state_dict(), args.out)
fresh = kpfcn.KPFCN(cfg)
fresh.load_state_dict(torch.load(args.out, map_location="cpu"), strict=True)
loss2, recall2 = evaluate(fresh.to(dev), held)
say(f"checkpoint {os.path.basename(args.out)} reloaded with strict=True: held-out descriptor loss {loss2:.4f}, recall {recall2:.3f} "
    f"({'the same numbers' if (loss2, recall2) == (loss1, recall1) else 'DIFFERENT numbers'})")
if args.log:
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")
