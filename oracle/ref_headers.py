"""Stages the reference's headers (kokkos-kernels: the directories its sparse/ interfaces include) into oracle/_ref/kokkos-kernels/,
the input of tests/test_tpl_binding.py, which compiles the drop-in binding (kokkos-kernels_amd/host/kokkos_tpl/) against them.
Called by __graft_entry__.build().  oracle/_ref/ stays out of version control: nothing of the reference is committed.  The source
checkout is taken from KK_REFERENCE_SRC (default: the build container's checkout); where there is none, nothing is staged and the
binding test says so when it skips."""
import os
import shutil

_HERE = os.path.dirname(os.path.abspath(__file__))
DEST = os.path.join(_HERE, "_ref", "kokkos-kernels")
# the include directories tests/test_tpl_binding.py compiles with (top-level headers of each, no sources or unit tests)
DIRS = ("sparse/src", "sparse/impl", "sparse/tpls", "common/src", "common/impl", "graph/src", "graph/impl",
        "blas/src", "blas/impl", "blas/tpls", "batched", "batched/dense/src", "batched/dense/impl")


def source():
    return os.environ.get("KK_REFERENCE_SRC", "/root/reference")


def stage():
    """copy the headers of DIRS from the reference checkout into DEST; returns DEST, or None when there is no checkout"""
    src = source()
    if not os.path.isdir(os.path.join(src, "sparse", "tpls")):
        return None
    for d in DIRS:
        out = os.path.join(DEST, d)
        os.makedirs(out, exist_ok=True)
        for f in sorted(os.listdir(os.path.join(src, d))):
            p = os.path.join(src, d, f)
            if os.path.isfile(p) and f.endswith((".hpp", ".h")):
                shutil.copyfile(p, os.path.join(out, f))
    return DEST


def staged():
    return os.path.isdir(os.path.join(DEST, "sparse", "tpls"))
