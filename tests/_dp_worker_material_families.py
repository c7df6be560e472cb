"""Worker of test_material_families_host.test_identify_two_ranks_match_single (gloo, CPU): the identified steps of the plate or the 3-D model
on two ranks.  argv: family ("plate" | "nc3d"), output file."""
import sys

import numpy as np
import torch
import torch.distributed as dist

from tests.test_material_families_host import dp_model, dp_train

dist.init_process_group("gloo")
rank = dist.get_rank()
m = dp_model(sys.argv[1])
dp_train(m)
c = torch.tensor([m.E, m.mu, m.rho], dtype=torch.float64)
both = [torch.zeros_like(c) for _ in range(2)]
dist.all_gather(both, c)
if rank == 0:
    np.savez(sys.argv[2], c0=both[0].numpy(), c1=both[1].numpy(), rec=np.array(m.material_rec))
dist.destroy_process_group()
