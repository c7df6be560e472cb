"""What the model classes share below the reference's method surface.

``ModelBase`` (elastic_wave.DeepHPM, plate_hole.PINN, navier_cauchy_3d.NavierCauchy3D): the data-parallel topology, the default engine, the
step's collective and its status check, row shards, checkpoints, the once-per-model finite-gradient probe and the call into the L-BFGS stage
(optim.lbfgs_stage).  Methods that act on a net take the engine and the parameter tensor as arguments: the plate class has three of each.

``ShardedSetsModel`` (DeepHPM, NavierCauchy3D): one net whose collocation set is sharded by rows and whose side sets (initial state, source,
boundaries) each fill one slot of the loss-sum buffer.  The two classes differ in the class-level constants only.
"""
from __future__ import annotations

import numpy as np
import torch

from .net_api import NetApi, read_checkpoint, write_checkpoint
from .optim import _col, device_array, device_column, evaluate_with_finite_gradient, lbfgs_stage, pack_params, unpack_params


class ModelBase(NetApi):
    def _init_topology(self, process_group, always_reduce, shard_as=None):
        self.pg = process_group
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            self.rank = torch.distributed.get_rank(self.pg)
            self.world = torch.distributed.get_world_size(self.pg)
        else:
            self.rank, self.world = 0, 1
        if shard_as is not None:
            # ``shard_as=(r, w)``: hold and evaluate rank r's share of a w-rank job WITHOUT the other ranks -- every set sharded by _shard, sums
            # weighted with the global 1/N, exactly what that rank executes per step (bench.py --rank-share; the collective is a separate switch)
            self.rank, self.world = int(shard_as[0]), int(shard_as[1])
        # ``always_reduce``: run the step's all-reduce even in a process group of one rank -- the collective branch (RCCL under the
        # "nccl" backend) then executes on a single GPU exactly as it does on eight, which is how the tests prove that path here
        self._reduce = (self.world > 1 and shard_as is None) or (bool(always_reduce) and torch.distributed.is_available() and torch.distributed.is_initialized())

    def _default_engine(self, layers, precision, n_collo):
        """the GPU engine of a net of ``layers``, its workspace sized for this rank's share of ``n_collo`` collocation points"""
        from .hip_engine import HipEngine
        return HipEngine(layers, precision=precision, max_points=max(int(n_collo) // self.world + 1, 1 << 14))

    def _set_engine(self, engine, family):
        """``engine``: the one behind ``self.theta`` (tests may inject a stand-in with the same methods); ``family``: its kernel family"""
        self.engine = engine
        self.device = engine.device
        if hasattr(engine, "warn_if_slow_path"):
            engine.warn_if_slow_path(family)      # no silent slow path: a depth the fused kernel is not compiled for says so once

    def _init_collective(self, collective, p2p_timeout_s):
        """``collective``: "rccl" (default) = torch.distributed.all_reduce of the fused buffer ``self._buf``; "p2p" = the library's one-shot
        all-reduce over IPC-mapped peer buffers with the Adam update in the same kernel (p2p.P2PAllReduce, include/pinn_hip.h: pinn_p2p_*)"""
        if collective not in ("rccl", "p2p"):
            raise ValueError("collective must be 'rccl' or 'p2p'")
        self._p2p = None
        if collective == "p2p" and self._reduce:
            if not hasattr(self.engine, "lib"):
                raise ValueError("collective='p2p' needs the HIP engine (the one-shot all-reduce is a kernel of libpinn_hip.so)")
            from .p2p import P2PAllReduce
            self._p2p = P2PAllReduce(self.engine.lib, self._buf.numel(), self.pg, timeout_s=p2p_timeout_s)

    def _check_collective(self):
        """collective='p2p': raise if a one-shot all-reduce has failed on this rank (p2p.P2PAllReduce.check: reads a host word, no
        synchronisation) -- called behind every host sync point of train / train_bfgs / getloss, so that a rank that missed a call, or whose
        peer did, stops at once instead of training on with diverged parameters (round-5 review)."""
        if getattr(self, "_p2p", None) is not None:
            self._p2p.check()

    def close(self):
        """Release the P2P communicator (collective: every rank calls it).  Nothing to do for collective='rccl'."""
        p2p, self._p2p = getattr(self, "_p2p", None), None
        if p2p is not None:
            p2p.close()

    def _shard(self, lo, hi):
        n = hi - lo
        return lo + n * self.rank // self.world, lo + n * (self.rank + 1) // self.world

    def _device_columns(self, cols, device=None):
        """host columns ([N,1] or [N]) -> fp32 device tensors [N]"""
        return [device_column(a, self.device if device is None else device) for a in cols]

    @staticmethod
    def _cols(T):
        return tuple(T[i].detach().cpu().numpy().reshape(-1, 1) for i in range(T.shape[0]))

    # ---- checkpoints: the reference's [W_list, b_list] pickle (INF:159-186); .npz is accepted too ---------------------------------------
    def _save_net(self, fileDir, theta, layers):
        W, b = unpack_params(theta.detach().cpu().numpy(), layers)
        write_checkpoint(fileDir, W, b, layers)
        if self.verbose:
            print("Save NN parameters successfully...")

    def save_NN(self, fileDir, TYPE=''):
        """INF:159-170.  A name ending in ``.npz`` writes plain arrays (the documented default of this package); any other name writes the
        reference's pickle of [W_list, b_list] (net_api.py)."""
        self._save_net(fileDir, self.theta, self.uv_layers)

    def load_NN(self, fileDir, layers):
        """INF:172-186: ``.npz`` or the reference's pickle (read by an arrays-only unpickler, net_api.py)"""
        num_layers = len(layers)
        uv_weights, uv_biases = read_checkpoint(fileDir)
        # Stored model must have the same number of layers (INF:178)
        assert num_layers == (len(uv_weights) + 1)
        weights = [np.asarray(w, dtype=np.float32) for w in uv_weights]
        biases = [np.asarray(b, dtype=np.float32).reshape(1, -1) for b in uv_biases]
        for i, w in enumerate(weights):
            assert w.shape == (layers[i], layers[i + 1]), "stored weight shape does not match the layers asked for"
        if self.verbose:
            print("Load NN parameters successfully...")
        return weights, biases

    # ---- what train / train_bfgs do around their evaluations ----------------------------------------------------------------------------
    def _settle_adjoint_shift(self, engine, evaluate, n_params):
        """In front of an Adam loop, once per model: a synchronous evaluation settles the adjoint shift (Adam's steps are small, it rarely
        moves after).  ``evaluate()`` fills and returns the device buffer [grad (n_params) | sums]."""
        if getattr(engine, "needs_finite_probe", False) and not self._shift_state.get("probed"):
            evaluate_with_finite_gradient(engine, evaluate, n_params, self._shift_state, check=self._check_collective)
            self._shift_state["probed"] = True

    def _lbfgs_stage(self, backend, engine, theta, evaluate, loss_of_sums, loss_coeffs, options):
        """optim.lbfgs_stage with this model's callback, collective check and adjoint-shift bookkeeping"""
        return lbfgs_stage(backend, engine, theta, evaluate, loss_of_sums, loss_coeffs, options, self.callback, self._check_collective,
                           self._shift_state)


class ShardedSetsModel(ModelBase):
    N_IN = 0                  # input columns of the net: the point sets' coordinate columns
    COLLO_NAMES = ()          # the attributes that keep the collocation set's host columns [N,1], as the reference does (INF:40-42)
    COLLO_TERMS = (0, 0)      # how many of the collocation residuals the layout weights with f_uv, then with f_s: together the net's outputs
    SUMS_STRIDE = 0           # floats per slot in the loss-sum buffer
    SLOTS = ()                # "collo", then the names of the side sets, in buffer order

    def _current_theta(self):
        return self.theta

    def _init_net(self, seed, ExistModel, modelDir):
        """weights (INF:64-68) as one flat device vector, and Adam's state"""
        self._init_rng = np.random.default_rng(seed)
        if ExistModel == 0:
            W, b = self.initialize_NN(self.uv_layers)
        else:
            W, b = self.load_NN(modelDir, self.uv_layers)
        self.n_params = sum(w.size for w in W) + sum(x.size for x in b)
        self.theta = torch.from_numpy(pack_params(W, b)).to(self.device)
        self._shift_state["theta"] = self.theta        # (updated in place: the weight-range check of evaluate_with_finite_gradient reads it)
        self.adam_m = torch.zeros_like(self.theta)
        self.adam_v = torch.zeros_like(self.theta)
        self.adam_t = 0

    def _init_collocation(self, Collo):
        Collo = np.asarray(Collo, dtype=np.float64)
        for k, name in enumerate(self.COLLO_NAMES):      # host copies, as the reference keeps them (INF:40-42)
            setattr(self, name, Collo[:, k:k + 1])
        # Device residency: one process holds the whole set; a data-parallel rank holds only ITS rows of each collocation block
        # (uploaded when a block is first used, see _rows), so device memory and upload time scale with 1/world.
        self._n_collo = Collo.shape[0]
        self._collo_host = tuple(np.ascontiguousarray(_col(Collo[:, k]), dtype=np.float32) for k in range(self.N_IN))
        self._collo_full = tuple(device_array(a, self.device) for a in self._collo_host) if self.world == 1 else None
        self._collo_cache = {}
        self._sides = {}      # name -> (N_IN coordinate columns, targets [outputs, n] or None, out columns, global row count)

    def _add_side(self, name, A, cols, target_cols=None):
        """Register the side set ``A`` [n, N_IN (+ target columns)] under the slot ``name``: this rank's rows on the device; the squared outputs
        ``cols`` (minus the columns ``target_cols`` of A, where given) enter its loss term."""
        if A is None:
            return
        A = np.asarray(A, dtype=np.float64)
        if A.shape[0] == 0:
            return
        n_glob = A.shape[0]
        s, e = self._shard(0, n_glob)            # this rank's contiguous rows
        A = A[s:e]
        tg = None
        if target_cols is not None and e > s:
            T = np.zeros((sum(self.COLLO_TERMS), A.shape[0]), dtype=np.float32)
            for o, cidx in zip(cols, target_cols):
                T[o] = A[:, cidx]
            tg = device_array(T, self.device)
        self._sides[name] = tuple(self._device_columns(A[:, k] for k in range(self.N_IN))) + (tg, tuple(cols), n_glob)

    def _rows(self, lo, hi):
        """Device tensors (one per coordinate) of THIS rank's rows of the collocation block [lo, hi)."""
        s, e = self._shard(lo, hi)
        if self._collo_full is not None:
            return tuple(a[s:e] for a in self._collo_full)
        key = (lo, hi)
        if key in self._collo_cache:
            self._collo_cache[key] = self._collo_cache.pop(key)          # most recently used last
        else:
            # Bounded cache, least recently used out first: TWICE this rank's share of the set stays resident, so that train() walking
            # its blocks and getloss() asking for (0, N) in between -- two batchings of the same rows -- alternate without re-uploading
            # a shard from the host every time, and shifting windows still cannot grow the device footprint beyond that bound.
            self._collo_cache[key] = tuple(torch.from_numpy(h[s:e]).to(self.device) for h in self._collo_host)
            cap = 2 * (-(-self._n_collo // self.world)) + 64
            while len(self._collo_cache) > 1 and sum(v[0].numel() for v in self._collo_cache.values()) > cap:
                del self._collo_cache[next(iter(self._collo_cache))]
        return self._collo_cache[key]

    @property
    def _collo(self):
        """this rank's rows of the whole collocation set"""
        return self._rows(0, self._n_collo)

    def _terms_from_sums(self, sums, n_blk):
        """sums: [len(SLOTS), SUMS_STRIDE] numpy array of sums of squares -> the reference's loss terms."""
        lay, n_uv, n_out = self.layout, self.COLLO_TERMS[0], sum(self.COLLO_TERMS)
        out = {"loss_f_uv": float(sums[0, :n_uv].sum() / n_blk), "loss_f_s": float(sums[0, n_uv:n_out].sum() / n_blk)}
        total = lay["f_uv"] * out["loss_f_uv"] + lay["f_s"] * out["loss_f_s"]
        for k, name in enumerate(self.SLOTS[1:], start=1):
            if name in self._sides:
                cols, n = self._sides[name][-2:]
                out["loss_" + name] = float(sums[k, list(cols)].sum() / n)
            else:
                out["loss_" + name] = 0.0
            total = total + lay[name] * out["loss_" + name]
        out["loss"] = total
        return out

    def _loss_coeffs(self, n_blk):
        """_terms_from_sums(...)["loss"] as a coefficient vector over the sums buffer (SUMS_STRIDE floats per slot): the loss is linear in it"""
        lay, n_uv, n_out = self.layout, self.COLLO_TERMS[0], sum(self.COLLO_TERMS)
        c = np.zeros((len(self.SLOTS), self.SUMS_STRIDE))
        c[0, :n_uv], c[0, n_uv:n_out] = lay["f_uv"] / n_blk, lay["f_s"] / n_blk
        for k, name in enumerate(self.SLOTS[1:], start=1):
            if name in self._sides:
                cols, n = self._sides[name][-2:]
                c[k, list(cols)] = lay[name] / n
        return c.reshape(-1).tolist()
