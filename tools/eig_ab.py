"""Interleaved same-process A/B of builds of pamnet_sym_eig_f64 (profiles/vib.txt): every library given on the command line is
loaded side by side through ctypes and the builds alternate inside each round on the same inputs; ms per call (the copy that restores
the consumed input included), and whether each build gives the bits of the first.  A variant build is csrc/eig.hip with another
constant (kStageMax = 0: the global-memory form for every d; kThreads; kColBatch / kRowBatch) compiled with build.FLAGS and linked
with the other objects of csrc/build.
Run on the GPU box: python tools/eig_ab.py LIB_A.so LIB_B.so [...]"""
import ctypes
import os
import statistics
import sys

import torch

dev = torch.device('cuda:0')
libs = {}
for path in sys.argv[1:]:
    lib = ctypes.CDLL(path)
    fn = lib.pamnet_sym_eig_f64
    fn.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_int64, ctypes.c_double, ctypes.c_int32, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    libs[os.path.basename(path)[:-3]] = fn
stream = torch._C._cuda_getCurrentRawStream(0)
torch.manual_seed(0)


def case(d, count, reps):
    m = torch.randn(count, d, d, dtype=torch.float64, device=dev)
    master = (m + m.transpose(1, 2)).reshape(-1).contiguous()
    dims = torch.full((count,), d, dtype=torch.long, device=dev)
    zero = torch.zeros(1, dtype=torch.long, device=dev)
    dptr, moff = torch.cat([zero, dims.cumsum(0)]), torch.cat([zero, (dims * dims).cumsum(0)])
    a, v = master.clone(), torch.zeros_like(master)
    w = torch.zeros(count * d, dtype=torch.float64, device=dev)
    st, sw = torch.zeros(count, dtype=torch.int32, device=dev), torch.zeros(count, dtype=torch.int32, device=dev)
    def run(fn):
        for _ in range(reps):
            a.copy_(master)
            rc = fn(a.data_ptr(), v.data_ptr(), w.data_ptr(), st.data_ptr(), sw.data_ptr(), moff.data_ptr(), dptr.data_ptr(), count,
                    1e-15, 30, stream)
            assert rc == 0
    return run, reps, w, st, sw


def timed(f):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


cases = {(9, 1): case(9, 1, 20), (54, 1): case(54, 1, 5), (87, 1): case(87, 1, 5), (192, 1): case(192, 1, 2), (87, 128): case(87, 128, 2),
         (54, 1024): case(54, 1024, 2)}
ref = {}
for c, (run, reps, w, st, sw) in cases.items():
    for name, fn in libs.items():
        run(fn)
        torch.cuda.synchronize()
        assert int(st.max()) == 0
        if c not in ref:
            ref[c] = w.clone()
        print(c, name, 'sweeps', int(sw.max()), 'same w bits as first', bool(torch.equal(ref[c], w)), flush=True)
t = {(c, n): [] for c in cases for n in libs}
for _ in range(7):
    for c, (run, reps, w, st, sw) in cases.items():
        for name, fn in libs.items():
            t[(c, name)].append(timed(lambda: run(fn)) / reps)
for c in cases:
    for name in libs:
        v = t[(c, name)]
        print('%4d x d=%3d  %-16s median_ms %8.3f  min %8.3f  max %8.3f' % (c[1], c[0], name, statistics.median(v), min(v), max(v)),
              flush=True)
