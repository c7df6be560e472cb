"""Worker of tests/test_gpu_causal_dp.py: ONE rank of a 2-process data-parallel run on a single GPU (both ranks on cuda:0, gloo for the
collective): one causal redraw of the rank's shard -- the probe points on the shared stream, the rows on the rank's own --, then two training
steps."""
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, ".")
from tests.test_gpu_refine import model                    # noqa: E402

dist.init_process_group("gloo")
torch.cuda.set_device(0)
rank = dist.get_rank()
N = 2001
m, _ = model([3] + 4 * [32] + [7], n_rows=N)
out = m.resample_collocation(dict(bins=16, eps=1.0, candidates=8192, exclude=[(15.0, 15.0, 2.0)], seed=77))
rec = {"cdf_": out["cdf"], "w_": out["w"], "counts_": out["counts"], "redrawn_": np.array(out["redrawn"]),
       "shard_": np.stack([a.cpu().numpy() for a in m._collo], axis=1)}
m.train(2, 1e-3, 1)
rec["theta_"] = m.theta.cpu().numpy()
gathered = [None, None]
dist.all_gather_object(gathered, rec)
if rank == 0:
    flat = {"n": np.array(N)}
    for r, g in enumerate(gathered):
        for k, v in g.items():
            flat[f"{k}{r}"] = v
    np.savez(sys.argv[1], **flat)
dist.barrier()
dist.destroy_process_group()
