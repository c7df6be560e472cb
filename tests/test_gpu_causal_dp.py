"""-m gpu: causal sampling on two data-parallel ranks (tests/_dp_worker_causal.py, driven as test_gpu_sample.py drives its worker)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _causal_cases as CC
from tests import _refine_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_two_ranks_get_the_same_table_and_disjoint_rows(tmp_path):
    """Two processes on one GPU (gloo for the collective).  The probe points share the stream 0x80000000 | round and the parameters are the
    same, so both ranks report the same table bytes with no collective; rank k draws its rows from stream k, so no point appears twice; the
    rows are this stream's points at that table; the parameters are still bit-identical across the ranks after two steps."""
    out = str(tmp_path / "dp_causal.npz")
    env = dict(os.environ, PYTHONPATH=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT="29567", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", "29567", os.path.join(ROOT, "tests", "_dp_worker_causal.py"), out], env=env, capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z = np.load(out)
    n = int(z["n"])
    assert z["cdf_0"].tobytes() == z["cdf_1"].tobytes() and z["w_0"].tobytes() == z["w_1"].tobytes() and np.array_equal(z["counts_0"], z["counts_1"])
    assert z["cdf_0"].shape == (17,) and z["cdf_0"][0] == 0 and z["cdf_0"][16] == 1 and (np.diff(z["cdf_0"]) >= 0).all()
    assert np.array_equal(z["theta_0"], z["theta_1"]) and np.isfinite(z["theta_0"]).all()
    shards = []
    for rank in (0, 1):
        lo, hi = n * rank // 2, n * (rank + 1) // 2
        S = z[f"shard_{rank}"]
        assert S.shape == (hi - lo, 3) and int(z[f"redrawn_{rank}"]) == hi - lo
        n_draw = (hi - lo) + (hi - lo) // 8 + 64
        P, _, t64 = CC.draw_reference(77, rank, 0, n_draw, RC.LB, RC.UB, z["cdf_0"])
        valid = (P[:, 0] - np.float32(15)) ** 2 + (P[:, 1] - np.float32(15)) ** 2 > np.float32(2) ** 2
        want, t64 = P[valid][:hi - lo], t64[valid][:hi - lo]
        assert (np.abs(S[:, :2] - want[:, :2]) <= np.spacing(np.abs(want[:, :2]))).all()         # this stream's points, no other's
        assert (np.abs(S[:, 2] - t64) <= CC.t_bound(RC.LB[2], RC.UB[2])).all()
        shards.append(S)
    allp = np.concatenate(shards)
    assert np.unique(allp, axis=0).shape[0] == allp.shape[0]
