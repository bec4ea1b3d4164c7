"""csrc/persistence.hip on the host, against exact arithmetic.  tests/host/pd_host.cpp compiles the per-cloud algorithm
(pd::pd_run, one lane) into a stand-alone program with the library's compiler and flags; the clouds of tests/pd_cases.py go through
it and tests/pd_exact.py referees the triangulation (integer predicates) and the diagram (rational filtration values).  A second
build of the same program under the address and undefined-behaviour sanitizers runs the same clouds and must stay silent."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import pd_cases, pd_exact
from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "host", "pd_host.cpp")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
# every cloud once, then the mixed sequence: the program reuses one workspace, so a cloud after a failed one sees its leftovers
ORDER = list(pd_cases.EXACT) + list(pd_cases.STATUS) + [n for n, _ in pd_cases.MIXED]


def compile_host(out, extra=()):
    from tgpose_amd import build
    subprocess.check_call([build.HIPCC] + build.FLAGS + list(extra) + ["-x", "hip", SRC, "-o", out])
    return out


def write_clouds(path, clouds, tet_cap=0):
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(clouds)))
        for pc in clouds:
            pc = np.ascontiguousarray(pc, dtype=np.float32)
            f.write(struct.pack("ii", len(pc), tet_cap))
            f.write(pc.tobytes())


def read_results(path, count):
    b = open(path, "rb").read()
    out, o = [], 0
    for _ in range(count):
        status, ntet, c1, c2 = struct.unpack_from("4i", b, o)
        o += 16
        r = dict(status=status, counts=(c1, c2))
        r["tets"] = np.frombuffer(b, np.int32, ntet * 4, o).reshape(-1, 4)
        o += ntet * 16
        r["h1"] = np.frombuffer(b, np.float64, c1 * 2, o).reshape(-1, 2)
        o += c1 * 16
        r["h2"] = np.frombuffer(b, np.float64, c2 * 2, o).reshape(-1, 2)
        o += c2 * 16
        out.append(r)
    assert o == len(b)
    return out


_plain = []


def plain_results(tmp_path_factory):
    """the plain program compiled once and run once over ORDER, however many test modules ask: (results, the output's bytes, the
    input file).  No sanitizer here: the device tests call this too."""
    if not _plain:
        d = tmp_path_factory.mktemp("pd_host")
        plain = compile_host(str(d / "pd_host"))
        write_clouds(str(d / "in.bin"), [pd_cases.cloud(n) for n in ORDER])
        subprocess.run([plain, str(d / "in.bin"), str(d / "out.bin")], check=True, timeout=600)
        _plain.append((read_results(str(d / "out.bin"), len(ORDER)), open(str(d / "out.bin"), "rb").read(), str(d / "in.bin")))
    return _plain[0]


@pytest.fixture(scope="session")
def host(tmp_path_factory):
    return plain_results(tmp_path_factory)


def check_exact_case(name, status, tets, h1, h2):
    """the checks the CPU and the GPU tests share: status 0, an exactly Delaunay triangulation, the exact diagram's pairs"""
    want_tets, keep1, keep2 = pd_cases.EXACT[name]
    pc = pd_cases.cloud(name)
    assert status == 0
    assert want_tets is None or len(tets) == want_tets, len(tets)
    pd_exact.check_triangulation(pc, tets)
    dg = pd_exact.exact_diagram(pc, tets)
    scale = max([d[:, 1].max() for d in dg.values() if len(d)] + [0.0])
    n_got = [len(pd_exact.kept(got, scale)) for got in (h1, h2)]
    n_want = [len(pd_exact.kept(dg[dim], scale)) for dim in (1, 2)]
    print("%s: %d tetrahedra; kept pairs above %.3g: H1 %d (exact %d), H2 %d (exact %d)"
          % (name, len(tets), pd_exact.PERS_FLOOR * scale, n_got[0], n_want[0], n_got[1], n_want[1]))
    for dim, got, keep in ((1, h1, keep1), (2, h2, keep2)):
        assert (got[:, 1] > got[:, 0]).all()
        lone_got, lone_want = pd_exact.match(got, dg[dim], scale)
        assert len(lone_got) == 0 and len(lone_want) == 0, ("H%d" % dim, lone_got[:4], lone_want[:4])
        assert n_want[dim - 1] == keep and n_got[dim - 1] == keep, ("H%d" % dim, n_got, n_want, keep)


@pytest.mark.parametrize("name", list(pd_cases.EXACT))
def test_host_matches_exact(host, name):
    r = host[0][ORDER.index(name)]
    check_exact_case(name, r["status"], r["tets"], r["h1"], r["h2"])


def check_status_case(name, status, ntet, counts):
    """the checks the CPU and the GPU tests share for a status cloud: the status, the tetrahedra and the pair counts of the table"""
    want_status, want_ntet, want_counts = pd_cases.STATUS[name]
    print("%s: status %d, %d tetrahedra, counts %r" % (name, status, ntet, counts))
    assert status == want_status
    assert want_ntet is None or ntet == want_ntet          # None: a cloud that overflowed the storage part-way
    assert tuple(counts) == want_counts
    if status == 0:
        assert ntet > 0 and ntet + 4 <= pd_cases.MAX_TETS


@pytest.mark.parametrize("name", list(pd_cases.STATUS))
def test_host_status(host, name):
    r = host[0][ORDER.index(name)]
    check_status_case(name, r["status"], len(r["tets"]), r["counts"])


def test_host_runs_do_not_depend_on_the_cloud_before(host):
    """a passing cloud after a failed one, in the same workspace, gives the bits it gave in its own place"""
    res = host[0]
    first = len(ORDER) - len(pd_cases.MIXED)
    ref = {}
    for k, (name, status) in enumerate(pd_cases.MIXED):
        r = res[first + k]
        assert r["status"] == status, name
        if status:
            assert r["counts"] == (0, 0), name
            continue
        assert len(r["h1"]) + len(r["h2"]) > 0
        ref.setdefault(name, r)
        for key in ("tets", "h1", "h2"):
            assert r[key].tobytes() == ref[name][key].tobytes(), (name, key)
    on = res[ORDER.index("on_grid")]
    assert on["tets"].tobytes() == res[first + 2]["tets"].tobytes() and on["h1"].tobytes() == res[first + 2]["h1"].tobytes()


def test_sanitizer_build_is_silent_and_agrees(host, tmp_path):
    """address + undefined-behaviour sanitizers on the host program, built and run here alone: exit 0, nothing on stderr, the plain
    build's bytes"""
    _, plain_bytes, clouds = host
    checked = compile_host(str(tmp_path / "pd_host_san"), SANITIZE)
    san = subprocess.run([checked, clouds, str(tmp_path / "out_san.bin")], capture_output=True, timeout=600)
    assert san.returncode == 0 and san.stderr == b"", san.stderr.decode(errors="replace")[-2000:]
    assert open(str(tmp_path / "out_san.bin"), "rb").read() == plain_bytes
