"""GPU: the first kernel launches of a process, made from several host threads at once (bench.py drives its bands that way), choose what a
single thread chooses.  The launch switches (launch_env.h), the CU count (pb_device_cus) and the LDS limits (pb_lds_limit) are all first
touched by these launches, so each run needs a fresh process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one 128 x 128 output tile over 16 K tiles on the generic tile, with a workspace lent: launch_gemm splits K (gemm.h splitk)
CHILD = """
import json, sys, threading
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import epi_ref as R
from prisma_amd import engine
n = %(threads)d
data = R.resid_data(7, 128, 128, 1024)
barrier = threading.Barrier(n)
raws, facts = [None] * n, [None] * n
def work(i):
    ops = engine.Ops(0)
    ops.set_option("op_splitk", 1)
    barrier.wait()
    raw, info, kname = ops.gemm_resid(*data, layout=R.MX2, tile=R.T_128)
    raws[i], facts[i] = raw, (info["splitk"], kname)
    ops.close()
th = [threading.Thread(target=work, args=(i,)) for i in range(n)]
for t in th: t.start()
for t in th: t.join()
assert all(r is not None for r in raws)
np.save(%(out)r, np.stack(raws))
print(json.dumps(facts))
"""


def child(tmp_path, threads):
    out = str(tmp_path / ("raw%d.npy" % threads))
    code = CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), threads=threads, out=out)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    return np.load(out), json.loads(r.stdout.strip().splitlines()[-1])


def test_first_launches_from_four_threads_equal_one_thread(tmp_path):
    """Four threads, each with its own ops context, meet at a barrier and make the process's first launch_gemm calls together: all report the
    split-K factor and the kernel, and return the bytes, of a second fresh process that launches from one thread.  Before the launch state
    was made thread-safe a thread could see the split-K limit published ahead of the CU count and launch unsplit; that window is a few
    instructions wide, so this test could not be made to fail reliably on the old code - it pins the behaviour, it does not hunt the race."""
    raw4, facts4 = child(tmp_path, 4)
    raw1, facts1 = child(tmp_path, 1)
    assert facts1[0][0] > 1 and facts1[0][1].startswith("gemm_kernel<128, 128, 2, 2, 0, 1,"), facts1
    assert all(f == facts1[0] for f in facts4), (facts4, facts1)
    for i in range(4):
        assert np.array_equal(raw4[i], raw1[0]), i
