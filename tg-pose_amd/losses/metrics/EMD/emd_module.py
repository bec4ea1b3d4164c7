"""Drop-in for ``losses/metrics/EMD/emd_module.py``: the auction approximation of the earth mover's distance.

``emdModule()(xyz1, xyz2, eps, iters) -> (dist (B,n) float32, assignment (B,n) int32)``: xyz1 the predicted cloud, xyz2 the
target, both (B,n,3) and normalised to [0,1]; ``sqrt(dist)`` is the distance of each point of xyz1 to the point of xyz2 it was
matched with.  The result is an approximation and the assignment need not be a bijection before the auction has converged.
Only xyz1 receives a gradient, as in the reference.

The reference's extension is CUDA, takes n % 1024 == 0 and B <= 512 only, and issues seven launches per iteration.  Here every
iteration runs inside ONE launch (``csrc/emd.hip``: a workgroup per cloud pair, the pair's state in LDS) for any
``1 <= n <= ops.emd_max_points()`` and any B; DESIGN.md "EMD" states the arithmetic."""
from torch import nn
from torch.autograd import Function

from .... import ops


class emdFunction(Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2, eps, iters):
        assert xyz1.size(1) == xyz2.size(1) and xyz1.size(0) == xyz2.size(0)
        xyz1 = xyz1.contiguous().float()
        xyz2 = xyz2.contiguous().float()
        dist, assignment = ops.emd_fwd(xyz1, xyz2, eps, iters)
        ctx.save_for_backward(xyz1, xyz2, assignment)
        ctx.mark_non_differentiable(assignment)
        return dist, assignment

    @staticmethod
    def backward(ctx, graddist, gradidx):
        xyz1, xyz2, assignment = ctx.saved_tensors
        gradxyz1 = ops.emd_bwd(xyz1, xyz2, graddist.contiguous().float(), assignment)
        return gradxyz1, xyz2.new_zeros(xyz2.shape), None, None


class emdModule(nn.Module):
    def forward(self, input1, input2, eps, iters):
        return emdFunction.apply(input1, input2, eps, iters)
