"""Worker of tests/test_gpu_refine_families.py: ONE rank of a 2-process data-parallel run on a single GPU (both ranks on cuda:0, gloo for the
collective): refine this rank's shard of a plate model's collocation set with this rank's own candidates, check that the frozen streams it holds
equal a fresh evaluation, then one training step."""
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, ".")
from tests import _refine_family_cases as FC                       # noqa: E402
from tests.test_gpu_refine_families import plate_model             # noqa: E402

dist.init_process_group("gloo")
torch.cuda.set_device(0)
rank = dist.get_rank()
N = 4001
m, _ = plate_model(n_rows=N)
lo, hi = m._shard(0, N)
cand = np.array(FC.plate_set(1500, 100 + rank))                    # rank-distinct candidates
s_rows = m.residual_score(m.x_c[lo:hi], m.y_c[lo:hi], m.t_c[lo:hi]).reshape(-1)
s_cand = m.residual_score(cand[:, 0:1], cand[:, 1:2], cand[:, 2:3]).reshape(-1)
out = m.refine_collocation(cand, 200)
held = m._frozen_collo.clone()
m.refresh_frozen()
assert held.shape == (2, 5, 5, hi - lo) and torch.equal(held.view(torch.int32), m._frozen_collo.view(torch.int32)), "frozen streams differ from a fresh evaluation"
m.train(1, 1e-3)
shard = np.stack([a.cpu().numpy() for a in m._collo], axis=1)
rec = dict(rows=out["rows"], cands=out["candidate_indices"], s_rows=s_rows, s_cand=s_cand, shard=shard, cand=cand.astype(np.float32),
           theta=m.theta["uv"].cpu().numpy())
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
