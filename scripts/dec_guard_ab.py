"""tgp_dec_l1, tgp_dec_fused and tgp_heads_fused at B = 32, N = 1028 under two or more builds of the library (an earlier commit's against
this tree's, say), alternating in ONE process on the same operand buffers, timed with the project's own timer (ops.GEMM_TIMER: HIP events
around each launch).   python scripts/dec_guard_ab.py <libtgpose_hip .so> <libtgpose_hip .so> [...]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tgpose_amd import _lib, ops  # noqa: E402

dev = "cuda:0"
B, N = 32, 1028
M = B * N
gen = torch.Generator().manual_seed(3)
d = lambda t: t.contiguous().to(dev)
rn = lambda *s: torch.randn(*s, generator=gen)
K = 268
fine = d(rn(M, 272))
Wa = rn(512, 272) / K ** 0.5
Wa[:, K:] = 0
Wa = d(Wa)
n1, n2 = M // 4, M // 16
P1, P2 = d(rn(n1, 640))[:, 128:], d(rn(n2, 640))[:, 128:]
idx1 = d(torch.randint(0, n1, (M,), generator=gen, dtype=torch.int32))
idx2 = d(torch.randint(0, n2, (M,), generator=gen, dtype=torch.int32))
rowbias = d(rn(B, 516) * 0.3)[:, :512]
vec1 = [d(rn(512) * 0.1), d(torch.rand(512, generator=gen) + 0.5), d(rn(512) * 0.1)]
Ws = [d(rn(n, k) / k ** 0.5) for n, k in ((512, 512), (256, 512), (128, 256))]
vecs = [(d(rn(n) * 0.1), d(torch.rand(n, generator=gen) + 0.5), d(rn(n) * 0.1)) for n in (512, 256, 128)]
w5, b5 = d(rn(3, 128) / 11.0), d(rn(3))
order = d(torch.stack([torch.randperm(N, generator=gen) for _ in range(B)]))
flag = torch.zeros(1, device=dev, dtype=torch.int32)
# the heads: tgp_heads_fused on the same features
WaH = rn(3072, 272) / K ** 0.5
WaH[:, K:] = 0
WaH = d(WaH)
HP1, HP2 = d(rn(n1, 3072)), d(rn(n2, 3072))
hb, hsc, hsh = d(rn(3072) * 0.1), d(torch.rand(3072, generator=gen) + 0.5), d(rn(3072) * 0.1)
HW2 = d(rn(3, 256, 1024) / 32.0)
hb2, hsc2, hsh2 = d(rn(3, 256) * 0.1), d(torch.rand(3, 256, generator=gen) + 0.5), d(rn(3, 256) * 0.1)

handles = {}
NAMES = [os.path.basename(a).replace("libtgpose_hip", "").replace(".so", "").strip("_") or "tree" for a in sys.argv[1:]]
for name, path in zip(NAMES, sys.argv[1:]):
    _lib._lib, _lib.LIB_PATH = None, os.path.abspath(path)
    handles[name] = _lib.lib()


def use(name):
    _lib._lib = handles[name]


outs = {}
state = {}
# ONE set of operand buffers for every library (the pack kernels are the same in all of them): only the code under test differs
use(NAMES[0])
shared = (ops.planes_split(fine, K=K), ops.heads_planes_w(Wa), ops.dec_pack(*Ws, h1_permuted=True), ops.Planes(M, 512, dev),
          ops.heads_planes_w(WaH), ops.heads_pack_w2(HW2, hb, hsc, hsh))
keys_buf, over_buf = torch.zeros(3, B, 256, device=dev, dtype=torch.int32), torch.zeros(1, device=dev, dtype=torch.int32)
out_buf = torch.empty(M, 3, device=dev)
for name in handles:
    state[name] = shared


def step(name):
    fp, wap, units, h1, hwa, hw2 = state[name]
    h1.amax.zero_()
    ops.dec_l1(fp, wap, P1, idx1, P2, idx2, *vec1, rowbias, N, h1, flag)
    out = ops.dec_fused(h1, units, vecs, w5, b5, order, N, flag, out=out_buf)
    keys_buf.zero_()
    keys, over = ops.heads_fused(fine, K, hwa, HP1, idx1, HP2, idx2, hw2, hb2, hsc2, hsh2, B, N, fine_planes=fp, keys=keys_buf, overflow=over_buf)
    keys = keys.clone()
    state["keys", name], state["over", name] = keys, over
    return out


for name in handles:
    use(name)
    for _ in range(30):
        outs[name] = step(name).clone()
torch.cuda.synchronize()
print("flag %d; outputs equal bit for bit: %s" % (int(flag.item()), [torch.equal(outs[n], outs[NAMES[0]]) for n in NAMES]))
ROUNDS, REPS = 12, 50
print("heads_fused: overflow flag %d, keys equal: %s" % (int(over_buf.item()), [torch.equal(state["keys", n], state["keys", NAMES[0]]) for n in NAMES]))
res = {n: {"dec_l1": [], "dec_fused": [], "heads_fused": []} for n in handles}
for rnd in range(ROUNDS):
    for name in NAMES[rnd % len(NAMES):] + NAMES[:rnd % len(NAMES)]:
        use(name)
        ops.GEMM_TIMER = []
        for _ in range(REPS):
            step(name)
        torch.cuda.synchronize()
        t = [e0.elapsed_time(e1) * 1e3 for e0, e1, *_ in ops.GEMM_TIMER]
        ops.GEMM_TIMER = None
        res[name]["dec_l1"].append(statistics.median(t[0::3]))
        res[name]["dec_fused"].append(statistics.median(t[1::3]))
        res[name]["heads_fused"].append(statistics.median(t[2::3]))
for k in ("dec_l1", "dec_fused", "heads_fused"):
    for name in NAMES:
        v = res[name][k]
        print("%-11s %-12s median of %d rounds (each the median of %d launches) %.1f us; rounds min %.1f max %.1f; all: %s"
              % (k, name, ROUNDS, REPS, statistics.median(v), min(v), max(v), " ".join("%.1f" % x for x in v)))
