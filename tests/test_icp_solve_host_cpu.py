"""csrc/icp_solve.h on the host: the point-to-plane solve that icp.hip and icp_dense.hip share, compiled into the stand-alone program
tests/host/icp_solve_host.cpp with the library's compiler and flags under the address and undefined-behaviour sanitizers, fed a few
6x6 systems -- regular, a plane's (three exact zero rows), singular, NaN, infinite -- and held to NumPy's solve of the same system."""
import os
import struct
import subprocess

import numpy as np

from tests import icp_ref
from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "host", "icp_solve_host.cpp")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]


def sums(rows, r):
    A, b = rows.T @ rows, rows.T @ r
    return np.concatenate([A[np.triu_indices(6)], b, [float(len(rows))]])


def systems():
    """-> list of (name, sums (28,), R, t, s, expected status)"""
    rng = np.random.default_rng(5)
    R0, t0 = icp_ref.rot([1, -2, 3], 25.0), np.array([0.1, -0.2, 0.9])
    q, n = rng.normal(size=(200, 3)), rng.normal(size=(200, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    rows = np.concatenate([np.cross(q, n), n], 1)
    out = [("regular", sums(rows, 0.01 * rng.normal(size=200)), R0, t0, 0.2, 0),
           ("tiny_step", sums(rows, 1e-9 * rng.normal(size=200)), R0, t0, 1.0, 0),          # the series branch of the exponential
           ("large_step", sums(rows, rows @ np.array([0.9, -0.4, 0.3, 0.1, 0.0, -0.2])), R0, t0, 1.0, 0)]
    flat = np.concatenate([np.cross(q * [1, 1, 0], [0, 0, -1.0]), np.tile([0, 0, -1.0], (200, 1))], 1)
    out.append(("plane", sums(flat, 0.003 + 0.01 * q[:, 0]), np.eye(3), np.array([0, 0, 1.0]), 1.0, 0))
    out.append(("zeros", np.zeros(28), R0, t0, 1.0, 2))
    bad = sums(rows, 0.01 * rng.normal(size=200))
    for name, where, value in (("nan_A", 3, np.nan), ("nan_b", 22, np.nan), ("inf_b", 25, np.inf), ("negative_pivot", 0, -1.0)):
        s = bad.copy()
        s[where] = value
        out.append((name, s, R0, t0, 1.0, 2))
    out.append(("inf_scale", out[0][1], R0, t0, np.inf, 2))
    return out


def numpy_solve(sm, R, t, s):
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = sm[:21]
    A = A + np.triu(A, 1).T
    A = A + np.eye(6) * (1e-9 * np.trace(A) / 6.0)
    x = np.linalg.solve(A, -sm[21:27])
    Rn = R @ icp_ref.rodrigues(x[:3]).T
    return Rn, t - s * (Rn @ x[3:]), float(np.linalg.norm(x[:3])), float(s * np.linalg.norm(x[3:])), x


def test_solve_plane_under_the_sanitizers(tmp_path):
    from tgpose_amd import build
    exe = str(tmp_path / "icp_solve_host")
    subprocess.check_call([build.HIPCC] + build.FLAGS + SANITIZE + ["-x", "hip", SRC, "-o", exe])
    cases = systems()
    with open(str(tmp_path / "in.bin"), "wb") as f:
        f.write(struct.pack("i", len(cases)))
        for _, sm, R, t, s, _ in cases:
            f.write(np.concatenate([sm, R.ravel(), t, [s]]).astype(np.float64).tobytes())
    done = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and "runtime error" not in done.stderr and "Sanitizer" not in done.stderr, done.stderr
    b = open(str(tmp_path / "out.bin"), "rb").read()
    assert len(b) == len(cases) * (4 + 14 * 8)
    for k, (name, sm, R, t, s, want) in enumerate(cases):
        status, = struct.unpack_from("i", b, k * 116)
        res = np.frombuffer(b, np.float64, 14, k * 116 + 4)
        assert status == want, (name, status)
        if status:
            assert res[2:11].tobytes() == R.ravel().tobytes() and res[11:14].tobytes() == t.tobytes(), name     # the state is untouched
            continue
        Rn, tn, ang, tr, x = numpy_solve(sm, R, t, s)
        print("%s: angle %.3e translation %.3e, max |dR| %.2e |dt| %.2e" % (name, res[0], res[1], np.abs(res[2:11] - Rn.ravel()).max(), np.abs(res[11:14] - tn).max()))
        assert np.abs(res[2:11] - Rn.ravel()).max() <= 1e-9 and np.abs(res[11:14] - tn).max() <= 1e-9, name
        assert abs(res[0] - ang) <= 1e-9 * max(1.0, ang) and abs(res[1] - tr) <= 1e-9 * max(1.0, tr), name
        Rm = res[2:11].reshape(3, 3)
        assert np.abs(Rm.T @ Rm - np.eye(3)).max() <= 1e-12, name
        if name == "plane":                                          # the three freedoms a plane leaves are solved to an exact 0
            assert x[2] == 0 and x[3] == 0 and x[4] == 0 and Rm[2, 2] != 1.0
