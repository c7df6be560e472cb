"""Worker of tests/test_gpu_lbfgs.py: ONE rank of a 2-process data-parallel run on a single GPU (both ranks on cuda:0, gloo for the collective)
through a backend="hip" L-BFGS stage: the all-reduced buffer [grad | sums] is the same on both ranks, the optimizer's kernels are deterministic,
so the parameters must stay bit-identical without any broadcast."""
import sys

import numpy as np
import torch
import torch.distributed as dist

from pinn_elastodynamics_amd.elastic_wave import DeepHPM
from pinn_elastodynamics_amd.hip_engine import HipEngine

sys.path.insert(0, ".")
from tests.test_gpu_dp import LAYERS, LB, UB, sets        # noqa: E402

dist.init_process_group("gloo")
torch.cuda.set_device(0)
dev = torch.device("cuda:0")
Collo, SRC, IC, UP = sets()
eng = HipEngine(LAYERS, precision="f16x3", device=dev, max_points=1 << 15)
m = DeepHPM(Collo, SRC, IC, UP, LAYERS, LB, UB, case="infinite", engine=eng, verbose=False, seed=9)
l0 = m.getloss()[0]
res = m.train_bfgs(1, options=dict(maxiter=20, maxfun=30, block=8), backend="hip")
l1 = m.getloss()[0]
th = [torch.zeros(m.n_params) for _ in range(dist.get_world_size())]
dist.all_gather(th, m.theta.cpu())
if dist.get_rank() == 0:
    np.savez(sys.argv[1], theta0=th[0].numpy(), theta1=th[1].numpy(), loss=np.array([l0, l1, res.fun]), counts=np.array([res.nfev, res.nit, m.count]))
dist.barrier()
dist.destroy_process_group()
