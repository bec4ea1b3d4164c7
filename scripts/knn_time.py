"""Development (GPU box): feature-space kNN timings at the forward's shapes (B = 32)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tgpose_amd import ops

dev = "cuda:0"
CALLS = 200
for (B, n, d, k) in ((32, 1028, 128, 20), (32, 257, 128, 20), (32, 257, 256, 20), (32, 64, 256, 8), (256, 1028, 128, 20)):
    x = torch.relu(torch.randn(B, n, d, device=dev) * 0.7 + 0.2)
    for _ in range(3):
        idx = ops.knn_feat(x, k)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        idx = ops.knn_feat(x, k)
    e1.record()
    torch.cuda.synchronize()
    print("knn_feat B=%d n=%d d=%d k=%d: %.1f us per call (prep + fused distance/selection)" % (B, n, d, k, e0.elapsed_time(e1) * 1e3 / CALLS), flush=True)
