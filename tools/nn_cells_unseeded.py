"""Time of ndp_chamfer_nn_cells (grid build + search, one pair, 200 calls between HIP events) without seeds -- a pair's first evaluation -- and
with the exact answer as seeds, on a config-A pair (synthetic_pair(0), 2000 samples each); NDP_HIP_LIB=<variant> times another build.
    python tools/nn_cells_unseeded.py          (profiles/nn_cells_unseeded.txt)"""
import os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _modes  # noqa: F401  (NDP_HIP_LIB)
from deformationpyramid_amd import ops
from deformationpyramid_amd.synthetic import synthetic_pair

dev = torch.device("cuda:0")
torch.manual_seed(0)
src, tgt, _, _ = synthetic_pair(0)
x = (src - src.mean(0))[torch.randperm(src.shape[0])[:2000]].contiguous().to(dev)
y = (tgt - tgt.mean(0))[torch.randperm(tgt.shape[0])[:2000]].contiguous().to(dev)
ref = ops.chamfer_nn(x, y)
for name, (px, py) in (("no seeds", (None, None)), ("exact seeds", (ref[1].clone(), ref[3].clone()))):
    out = ops.chamfer_nn_cells(x, y, px, py)
    assert all(torch.equal(a, b) for a, b in zip(out, ref))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200):
        ops.chamfer_nn_cells(x, y, px, py)
    e1.record()
    torch.cuda.synchronize()
    print(f"{os.environ.get('NDP_HIP_LIB', 'product').split('/')[-1]:14s} {name:12s} {e0.elapsed_time(e1) / 200 * 1000:7.1f} us per call")
