"""TEST INFRASTRUCTURE: a numpy Backend bound to tests/emu/libkkamd_emu.so -- the same kernel sources
as the product, compiled by g++ against the SIMT emulator (kk_emu.h).  Lets `-m "not gpu"` tests check
kernel logic (tiling, carries, hash tables, scans, sorts) on a machine without a GPU.  It is NOT a CPU
fallback of the product: nothing under kokkos-kernels_amd/ can load it."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import kk_loader

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "libkkamd_emu.so")
LOCK = os.path.join(HERE, ".build.lock")
_BACKEND = None


def build():
    # several processes may ask at once (the ranks of a multi-process test): one runs make, the others wait for it and find
    # the library up to date, instead of writing the same objects concurrently
    with open(LOCK, "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-C", HERE, "-s"])
    return SO


def backend():
    global _BACKEND
    if _BACKEND is None:
        kk = kk_loader.load()
        build()
        lib = kk._capi.bind(C.CDLL(SO))
        _BACKEND = kk.Backend(lib, lambda n, dt: np.zeros(int(n), dtype=dt),
                              lambda a: None if a is None else a.ctypes.data, lambda: None,
                              lambda a: a, lambda a: np.array(a, copy=True), "emu")
    return _BACKEND
