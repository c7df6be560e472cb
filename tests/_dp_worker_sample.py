"""Worker of tests/test_gpu_sample.py: ONE rank of a 2-process data-parallel run on a single GPU (both ranks on cuda:0, gloo for the collective):
two refinement rounds with candidates drawn on the device -- no stream given, so round * world + rank picks it --, then one training step."""
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, ".")
from tests.test_gpu_refine import model                    # noqa: E402

dist.init_process_group("gloo")
torch.cuda.set_device(0)
rank = dist.get_rank()
N = 4001
m, _ = model([3] + 4 * [32] + [7], n_rows=N)
rec = {}
for rnd, select in enumerate(("top", "sample")):
    out = m.refine_collocation(3000, 200, seed=77, select=select, exclude=[(15.0, 15.0, 2.0)])
    rec.update({f"rows_{rnd}_": out["rows"], f"idx_{rnd}_": out["candidate_indices"], f"pts_{rnd}_": out["candidates"]})
m.train(1, 1e-3, 1)
rec["shard"] = np.stack([a.cpu().numpy() for a in m._collo], axis=1)
rec["theta"] = m.theta.cpu().numpy()
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
