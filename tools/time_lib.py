"""Warm kernel times of one library build, for same-box A/B runs (run it alternately per build): k_secp_mul<0> at 2^N,
two warm-up launches, then K timed ones (HIP events inside the library).

    python tools/time_lib.py <path to libfecgpu.so> <log2 n> <K>
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from forge_ec_amd import _lib
_lib.SO_PATH = os.path.abspath(sys.argv[1])
import forge_ec_amd as F
import vectors as V
logn, K = int(sys.argv[2]), int(sys.argv[3])
n = 1 << logn
ctx = F.Context(0); ctx.set_timing(True)
k = V.scalars(n, 0, 1); p = V.points(n, 0, 2)
dk = torch.from_numpy(k.view(np.int64)).cuda(); dp = torch.from_numpy(p.view(np.int64)).cuda(); do = torch.empty_like(dp)
st = torch.cuda.current_stream().cuda_stream
ms = []
for r in range(K + 2):
    ctx.batch_mul_dev(0, dk.data_ptr(), dp.data_ptr(), do.data_ptr(), n, st)
    t, name = ctx.last_kernel_ms()
    if r >= 2: ms.append(t)
print("TIME %s 2^%d median %.3f min %.3f n=%d all %s" % (os.path.basename(sys.argv[1]), logn, float(np.median(ms)), min(ms), len(ms), " ".join("%.3f" % x for x in ms)), flush=True)
