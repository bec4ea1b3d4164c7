"""Builds tg-pose_amd/libtgpose_hip.so for gfx950 with hipcc (cross-compiles without a GPU).

    python -m tgpose_amd.build          # or: from tgpose_amd.build import build; build()

Flags that matter:
  --offload-arch=gfx950   the only target (CDNA4 / MI355X)
  -ffp-contract=off       the kNN / Chamfer kernels mirror the CPU path's fp32 rounding exactly;
                          fused multiply-adds appear only where written (fmaf, MFMA)
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SOURCES = ["knn.hip", "gemm.hip", "gemm_pp.hip", "gconv.hip", "chamfer.hip", "dcd.hip", "emd.hip", "fps.hip", "render.hip", "meshsample.hip", "ballcrop.hip", "icp.hip", "icp_dense.hip", "plane.hip", "segment.hip", "verify.hip", "meshmaps.hip", "poseerr.hip", "vsd.hip", "search.hip", "tsdf.hip", "weld.hip", "raycast.hip", "bn.hip", "backward.hip", "gconv_bwd.hip", "evalmetrics.hip", "tdaloss.hip", "inputside.hip", "rowsort.hip", "heads_fused.hip", "dec_fused.hip", "hs_chain.hip", "segsum.hip", "graph_bwd.hip", "poserot.hip", "gemm_tn_split.hip", "ranger.hip", "augment.hip", "persistence.hip", "xyz_bwd.hip", "draws.hip", "version.hip"]
DEV_SOURCES = ["gemm_variants.hip"]     # development build only (--dev): micro-benchmark kernels + the tgp_debug_* switches
LIB = os.path.join(HERE, "libtgpose_hip.so")
DEV_LIB = os.path.join(HERE, "libtgpose_hip_dev.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-Wall", "-Wno-unused-variable", "-Wno-unused-function"]


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))] + [os.path.join(os.path.dirname(HERE), "include", "tgpose.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True, dev=False):
    """dev=True: libtgpose_hip_dev.so with -DTGP_DEV (kernel-variant switches for scripts/*_ab.py; never loaded by the
    package itself -- a script points tgpose_amd._lib.LIB_PATH at it before the first call)."""
    if dev == "bnscalar":      # A/B measurement build: BatchNorm passes on the scalar kernels
        return _build(os.path.join(HERE, "libtgpose_hip_bnscalar.so"), SOURCES, ["-DTGP_BN_SCALAR"], ".bs.o", verbose)
    if dev == "predbig":       # A/B measurement build: predicated (repair) launches on the large tile shapes, as before round 4
        return _build(os.path.join(HERE, "libtgpose_hip_predbig.so"), SOURCES, ["-DTGP_PRED_BIG"], ".pb.o", verbose)
    if dev == "searchpad":     # A/B measurement build: the pose search's field rows padded by 4 bytes in LDS (scripts/search_pad_ab.py)
        return _build(os.path.join(HERE, "libtgpose_hip_searchpad.so"), SOURCES, ["-DTGP_SEARCH_PAD=4"], ".sp.o", verbose)
    if dev == "noguard":       # A/B measurement build: the product library without the fp16 range guard of the split GEMM
        return _build(os.path.join(HERE, "libtgpose_hip_noguard.so"), SOURCES, ["-DTGP_NO_RANGE_GUARD"], ".ng.o", verbose)
    if dev:
        return _build(DEV_LIB, SOURCES + DEV_SOURCES, ["-DTGP_DEV"], ".dev.o", verbose)
    if not force and not _stale():
        return LIB
    return _build(LIB, SOURCES, [], ".o", verbose)


def _build(LIB, sources, extra, suffix, verbose):
    """compile the sources whose object is older than the source or a header (in parallel: hipcc is one process per file), link"""
    from concurrent.futures import ThreadPoolExecutor
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [os.path.join(os.path.dirname(HERE), "include", "tgpose.h")]
    newest_hdr = max(os.path.getmtime(h) for h in hdrs)
    objs, todo = [], []
    for src in sources:
        obj = os.path.join(CSRC, src.replace(".hip", suffix))
        objs.append(obj)
        path = os.path.join(CSRC, src)
        if not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(path), newest_hdr):
            todo.append([HIPCC] + FLAGS + extra + ["-c", path, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(run, todo))
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv, dev="searchpad" if "--searchpad" in sys.argv else "predbig" if "--predbig" in sys.argv else "noguard" if "--noguard" in sys.argv else "bnscalar" if "--bnscalar" in sys.argv else "--dev" in sys.argv)
