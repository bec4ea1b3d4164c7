"""ops.DistanceFields and ops.pose_search (csrc/search.hip) against the NumPy restatement tests/search_ref.py: the field's bytes, the
whole per-rotation table, cost, rot and shift are EQUAL (everything after the floor is an integer); poses agree within 1e-6.

Models of 1, 100 and 2048 points in one set; G = 16 and 48 (G = 48 needs the LDS opt-in); twelve jobs in every call: n = 1, 63, 64,
65, 257 and 1024 live rows of a 1024-row cloud (the rows behind are finite rubbish that must count for nothing) with NaN and inf
rows inside, a cloud four times the cube's size (b + d leaves the grid on every side), an empty job and a far-away job (every
cost equal: both tie rules decide everything), a duplicated rotation (equal costs: the lower index first), and job_model = -1, M
and a count above n_cap (refused rows).  R = 1, 7 and 65 (a rotation block is 8), K = 0, 1, 2 with stride 1 and 3, top = 1, R, R + 3."""
import numpy as np
import pytest
import torch

from tests import search_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = 32
N_CAP = 1024
COUNTS_MODEL = [1, 100, 2048]
_S = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (run with -m gpu on the MI355X box)")


def rotations():
    from tgpose_amd.tools.lynne_lib import view_sampler
    Rs = view_sampler.rotation_grid(12, 6)[:65].copy()
    Rs[5] = Rs[3]
    return Rs


def host_models():
    r = np.random.RandomState(11)
    pn = np.zeros((3, 2048, 6), dtype=np.float32)
    pn[:, :, :3] = 7.0                                             # rows beyond a model's count: never read
    pn[0, 0, :3] = [0.1, -0.2, 0.3]
    pn[1, :100, :3] = r.uniform(-0.5, 0.5, (100, 3)) * [1.0, 0.6, 0.8]
    u = r.randn(2048, 3)
    pn[2, :, :3] = 0.4 * u / np.linalg.norm(u, axis=1, keepdims=True) * [1.0, 0.7, 0.5] + [0.05, 0.0, -0.02]
    return pn


def host_jobs(pn, Rs):
    """-> clouds (J,1024,3), counts, job_model, anchors, scales"""
    r = np.random.RandomState(12)
    live = [1, 63, 64, 65, 257, 1024]
    J = len(live) + 6
    clouds = r.uniform(-3.0, 3.0, (J, N_CAP, 3)).astype(np.float32)            # the rubbish behind the counts
    counts = np.zeros(J, dtype=np.int32)
    job_model = np.zeros(J, dtype=np.int32)
    anchors = np.zeros((J, 3), dtype=np.float32)
    scales = np.zeros(J, dtype=np.float32)

    def place(j, m, n, s, spread=1.0):
        src = pn[m, :COUNTS_MODEL[m], :3].astype(np.float64)
        y = src[r.randint(0, len(src), n)] * spread + r.randn(n, 3) * 0.01
        R = Rs[r.randint(len(Rs))].astype(np.float64)
        t = np.array([0.1, -0.05, 0.9]) + r.randn(3) * 0.05
        clouds[j, :n] = (s * y @ R.T + t).astype(np.float32)
        counts[j], job_model[j], scales[j] = n, m, s
        if n:
            anchors[j] = clouds[j, :n].astype(np.float64).mean(0).astype(np.float32) + (r.randn(3) * 0.01).astype(np.float32)
    for j, n in enumerate(live):
        place(j, (1, 2, 1, 2, 0, 2)[j], n, 0.1 + 0.02 * j)
    clouds[2, 5], clouds[2, 17, 1] = np.nan, np.inf
    clouds[4, ::7, 2] = np.nan
    clouds[5, 1000:1010] = -np.inf
    j = len(live)
    place(j, 1, 300, 0.2, spread=4.0)                             # four times the cube: out on every side
    place(j + 1, 2, 0, 0.15)                                      # no point: every cost 0
    anchors[j + 1] = [0.0, 0.0, 1.0]
    place(j + 2, 1, 50, 0.1)
    anchors[j + 2] += 5.0                                         # far away: every cost cap * 50
    place(j + 3, 1, 40, 0.1)
    job_model[j + 3] = -1
    place(j + 4, 2, 40, 0.1)
    job_model[j + 4] = 3
    place(j + 5, 1, 40, 0.1)
    counts[j + 5] = N_CAP + 1
    return clouds, counts, job_model, anchors, scales


def setup():
    if _S:
        return _S
    from tgpose_amd import ops
    pn = host_models()
    Rs = rotations()
    models = ops.IcpModels(torch.from_numpy(pn).to(DEV), COUNTS_MODEL)
    clouds, counts, job_model, anchors, scales = host_jobs(pn, Rs)
    _S.update(pn=pn, Rs=Rs, models=models, host=(clouds, counts, job_model, anchors, scales),
              dev=tuple(torch.from_numpy(x).to(DEV) for x in (clouds, counts, job_model, anchors, scales)), Rs_dev=torch.from_numpy(Rs).to(DEV),
              fields={}, ref_fields={})
    return _S


def fields(G):
    s = setup()
    if G not in s["fields"]:
        from tgpose_amd import ops
        s["fields"][G] = ops.DistanceFields(s["models"], G=G, cap=CAP)
        torch.cuda.synchronize()
    return s["fields"][G]


def ref_field(G, m):
    s = setup()
    if (G, m) not in s["ref_fields"]:
        s["ref_fields"][(G, m)] = sr.build_field(s["pn"][m, :COUNTS_MODEL[m], :3], G, CAP)
    return s["ref_fields"][(G, m)]


# the 2048-point model at G = 48 would take the restatement a minute: each size and each G is covered, not their product
@pytest.mark.parametrize("G,m", [(16, 0), (16, 1), (16, 2), (48, 0), (48, 1)])
def test_field_bytes(G, m):
    f = fields(G)
    want, meta, thr = ref_field(G, m)
    assert np.array_equal(f.meta_host[m], meta) and np.array_equal(f.thresholds[m].cpu().numpy(), thr)
    got = f.field[m].cpu().numpy()
    print("G %d model %d: levels %d..%d, %d bytes differ" % (G, m, want.min(), want.max(), (got != want).sum()))
    assert got.dtype == np.uint8 and got.shape == (G, G, G) and np.array_equal(got, want)
    torch.cuda.synchronize()


def reference(G, R, K, stride, top):
    s = setup()
    clouds, counts, job_model, anchors, scales = s["host"]
    out = []
    for j in range(len(clouds)):
        m = int(job_model[j])
        mm = m if 0 <= m < 2 or (m == 2 and G == 16) else 1        # a refused job reads no field; model 2 has no G = 48 restatement
        fld, meta, _ = ref_field(G, mm)
        out.append(sr.search(fld, meta, CAP, clouds[j], int(counts[j]), anchors[j], scales[j], s["Rs"][:R], K, stride, top, n_models=3, job_model=m))
    return {k: np.stack([o[k] for o in out]) for k in out[0]}


def call(G, R, K, stride, top, jobs=None):
    from tgpose_amd import ops
    s = setup()
    clouds, counts, job_model, anchors, scales = s["dev"] if jobs is None else tuple(x[jobs].contiguous() for x in s["dev"])
    return ops.pose_search(fields(G), job_model, clouds, counts, anchors, scales, s["Rs_dev"][:R], K=K, stride=stride, top=top, return_table=True)


def check(got, want, what):
    for k in ("table", "cost", "rot", "shift"):
        g = got[k].cpu().numpy()
        assert g.dtype == np.int32 and g.shape == want[k].shape, (what, k)
        assert np.array_equal(g, want[k]), (what, k, np.argwhere(g != want[k])[:5])
    p = got["poses"].cpu().numpy()
    assert np.array_equal(np.isnan(p), np.isnan(want["poses"])), what
    assert np.allclose(p, want["poses"], rtol=0, atol=1e-6, equal_nan=True), what


CASES = [(16, 65, 2, 1, 16), (16, 65, 1, 3, 1), (16, 7, 1, 3, 7), (16, 1, 1, 1, 4), (48, 7, 2, 3, 10), (48, 1, 0, 1, 1), (48, 65, 2, 1, 64)]


@pytest.mark.parametrize("G,R,K,stride,top", CASES)
def test_search_equals_the_restatement(G, R, K, stride, top):
    s = setup()
    jobs = None
    if G == 48:                                                    # the jobs of model 2 are left out (no restatement of its G = 48 field)
        jobs = torch.tensor([j for j, m in enumerate(s["host"][2]) if m != 2], device=DEV)
    got = call(G, R, K, stride, top, jobs)
    torch.cuda.synchronize()
    want = reference(G, R, K, stride, top)
    if jobs is not None:
        want = {k: v[jobs.cpu().numpy()] for k, v in want.items()}
    check(got, want, (G, R, K, stride, top))
    cost, rot, shift = want["cost"], want["rot"], want["shift"]
    hm = s["host"][2] if jobs is None else s["host"][2][jobs.cpu().numpy()]
    hc = s["host"][1] if jobs is None else s["host"][1][jobs.cpu().numpy()]
    refused = (hm < 0) | (hm > 2) | (hc > N_CAP)
    assert refused.sum() == 3 and (cost[refused] == sr.REFUSED).all() and (rot[refused] == -1).all() and (shift[refused] == -1).all()
    assert (cost[~refused][:, :min(top, R)] != sr.REFUSED).all() and (cost[:, R:] == sr.REFUSED).all()
    empty = np.flatnonzero((hc == 0) & ~refused)
    assert len(empty) == (1 if jobs is None else 0)
    for j in empty:                                                # every cost 0: shift 0 and the rotations in index order
        assert (cost[j, :min(top, R)] == 0).all() and (shift[j, :min(top, R)] == 0).all() and rot[j, :min(top, R)].tolist() == list(range(min(top, R)))
    if R > 5:                                                      # rotation 5 is rotation 3: equal rows, 3 ranked first
        t = want["table"]
        assert np.array_equal(t[:, 3], t[:, 5])
    torch.cuda.synchronize()


def test_the_grid_is_left_on_every_side():
    """the premise of the big cloud: at the best shift of its best rotation, bases lie below 0 and at or above G on each axis"""
    s = setup()
    clouds, counts, job_model, anchors, scales = s["host"]
    j = 6
    _, meta, _ = ref_field(16, 1)
    b, live = sr.bases(clouds[j], int(counts[j]), anchors[j], scales[j], meta[3], 16, s["Rs"][:7])
    for a in range(3):
        assert (b[:, live, a] < -2).any() and (b[:, live, a] >= 18).any()


def test_repeatable_and_graph_capturable():
    args = (16, 65, 2, 1, 16)
    a, b = call(*args), call(*args)
    for k in a:
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call(*args)
    for k, v in out.items():
        v.fill_(7 if v.dtype != torch.float32 else 7.0)
    g.replay()
    torch.cuda.synchronize()
    for k in a:
        assert out[k].cpu().numpy().tobytes() == a[k].cpu().numpy().tobytes(), k
    big = (48, 65, 2, 1, 64)
    jobs = torch.tensor([0, 2, 6], device=DEV)
    c, d = call(*big, jobs), call(*big, jobs)
    for k in c:
        assert c[k].cpu().numpy().tobytes() == d[k].cpu().numpy().tobytes(), k
    torch.cuda.synchronize()


def test_wrapper_refusals():
    from tgpose_amd import ops
    s = setup()
    clouds, counts, job_model, anchors, scales = s["dev"]
    Rs = torch.from_numpy(s["Rs"]).to(DEV)
    f = fields(16)
    with pytest.raises(TypeError):
        ops.pose_search(s["models"], job_model, clouds, counts, anchors, scales, Rs)
    with pytest.raises(ValueError, match="top"):
        ops.pose_search(f, job_model, clouds, counts, anchors, scales, Rs, top=65)
    with pytest.raises(ValueError, match="K"):
        ops.pose_search(f, job_model, clouds, counts, anchors, scales, Rs, K=17)
    with pytest.raises(ValueError, match="anchors"):
        ops.pose_search(f, job_model, clouds, counts, anchors[:3], scales, Rs)
    with pytest.raises(ValueError, match="G must"):
        ops.DistanceFields(s["models"], G=24)
    torch.cuda.synchronize()
