"""scan_dbscan_prepare (norms + pairwise-distance GEMM with its fp64 re-check + core test) at the workload size, 31 k points of
256 dimensions, in device events -- for one or more builds of the library side by side, each loaded by ctypes alone so that an
older build without the newer symbols loads too.  Two inputs: the Gaussian blobs of tools/dbscan_time.py and workload-like points
(non-negative, sparse, on rays out of the origin).  The adjacency bit matrices of all builds are compared through a checksum.
usage: python tools/dbscan_prepare_time.py LIB [LIB ...]"""
import ctypes
import sys

import torch

dev = torch.device("cuda")
n, D = 31000, 256
g = torch.Generator().manual_seed(n)
centers = torch.randn(64, D, generator=g) * 2
blobs = (centers[torch.randint(0, 64, (n,), generator=g)] + torch.randn(n, D, generator=g) * 0.12).to(dev)
real = torch.relu(torch.randn((n + 7) // 8, D, generator=g)) * 2
real = real.repeat_interleave(8, 0)[:n] * (0.05 + 0.95 * torch.rand(n, 1, generator=g))
real = real[torch.randperm(n, generator=g)].contiguous().to(dev)
libs = {}
for path in sys.argv[1:]:
    L = ctypes.CDLL(path)
    L.scan_dbscan_ws_bytes.restype = ctypes.c_int64
    L.scan_dbscan_ws_bytes.argtypes = [ctypes.c_int64]
    L.scan_dbscan_prepare.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_int32,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.scan_tune.argtypes = [ctypes.c_char_p, ctypes.c_int]
    libs[path] = L
nbytes = libs[sys.argv[1]].scan_dbscan_ws_bytes(n)
ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
info = torch.empty(2, dtype=torch.int32, device=dev)
sums = {}
for rep in range(3):
    for path, L in libs.items():
        for name, x in (("blobs", blobs), ("real-like", real)):
            for mode in (1, 0):
                L.scan_tune(b"dbscan_bf16x3", mode)
                ts = []
                for it in range(7):  # the first two are warm-up
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    rc = L.scan_dbscan_prepare(x.data_ptr(), n, D, 3.0, 5, ws.data_ptr(), info.data_ptr(), None)
                    b.record()
                    torch.cuda.synchronize()
                    assert rc == 0
                    ts.append(a.elapsed_time(b))
                ts = sorted(ts[2:])
                bits = ws[: n * ((n + 127) // 128 * 4) // 2].view(torch.int64).sum().item()
                print("rep %d %-40s %-9s gemm=%-6s prepare median %.3f ms (min %.3f max %.3f) first_core %d bits-checksum %d" % (
                    rep, path, name, "bf16x3" if mode else "fp32", ts[len(ts) // 2], ts[0], ts[-1], int(info[0]), bits), flush=True)
                sums.setdefault((name, mode), set()).add(bits)
assert all(len(v) == 1 for v in sums.values()), "adjacency bits differ between libraries"
print("adjacency bit matrices identical across libraries and repetitions")
