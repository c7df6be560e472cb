"""CPU tests of the host side of device-drawn candidates, excluded regions and select="sample" (no library): a stand-in engine that draws, scores,
forms keys and selects in numpy -- tests/test_refine_host.RefineEngine plus sample_box / refine_keys from the references of tests/_sample_cases.py."""
import numpy as np
import pytest
import torch

from pinn_elastodynamics_amd.elastic_wave import DeepHPM, DeepHPMConfined
from pinn_elastodynamics_amd.refine import RefineSchedule, pair_by_key
from tests import _refine_cases as RC
from tests import _sample_cases as SC
from tests.test_refine_host import LAYERS, RefineEngine, sets


class SamplingEngine(RefineEngine):
    """RefineEngine with HipEngine's sample_box / refine_keys: the numpy references"""

    def sample_box(self, n, lo, hi, seed, stream=0, first=0):
        self.calls.append(("sample_box", int(n), int(seed), int(stream), int(first), tuple(lo), tuple(hi)))
        P = SC.box64(seed, stream, first, n, lo, hi).astype(np.float32)
        return tuple(torch.from_numpy(np.ascontiguousarray(P[:, k])) for k in range(P.shape[1]))

    def refine_keys(self, score, cols, balls=(), mode="mask", power=1.0, c=1.0, seed=0, stream=0, first=0):
        self.calls.append(("keys", score.numel(), tuple(balls), mode, float(power), float(c), int(seed), int(stream)))
        xs = [a.numpy() for a in cols]
        inside = SC.in_balls(xs, [(tuple(b[:-1]) + (0.0,) * (4 - len(b)), b[-1], len(b) - 1, 0) for b in balls])
        s = score.numpy()
        if mode == "mask":
            return torch.from_numpy(np.where(inside, np.float32(-np.inf), s))
        key, _ = SC.keys_reference(s, inside, power, c, SC.noise_u(seed, stream, first, s.size), np.float32)
        return torch.from_numpy(key.astype(np.float32))


def wave(rank=0, world=1, n=120):
    Collo, SRC, IC, UP = sets(n)
    eng = SamplingEngine(LAYERS)
    if world == 1:
        return DeepHPM(Collo, SRC, IC, UP, LAYERS, RC.LB, RC.UB, engine=eng, verbose=False, seed=3), eng, Collo
    return DeepHPMConfined(Collo.copy(), SRC, IC, UP, None, LAYERS, None, None, RC.LB, RC.UB, engine=eng, verbose=False, seed=3,
                           shard_as=(rank, world)), eng, Collo


def test_pair_by_key_orders_by_key_and_keeps_by_score():
    t = lambda v, dt=torch.float32: torch.tensor(v, dtype=dt)
    ninf = float("-inf")
    # candidates 2, 5, 7: keys 0.1, 9, -inf; scores 8, 2, 50.  rows 0, 1, 3 with scores 1, 3, 0 -> ascending: row 3 (0), row 0 (1), row 1 (3)
    r, c, rs, cs = pair_by_key(t([2, 5, 7], torch.int64), t([0.1, 9.0, ninf]), t([8.0, 2.0, 50.0]), t([0, 1, 3], torch.int64), t([1.0, 3.0, 0.0]))
    # pairs by key: (cand 5: score 2, row 3: 0) kept; (cand 2: 8, row 0: 1) kept; (cand 7: excluded) never, though 50 > 3
    assert r.tolist() == [3, 0] and c.tolist() == [5, 2] and rs.tolist() == [0.0, 1.0] and cs.tolist() == [2.0, 8.0]
    # a candidate whose score is not strictly larger stays out, whatever its key
    r, c, _, _ = pair_by_key(t([1], torch.int64), t([100.0]), t([1.0]), t([0], torch.int64), t([1.0]))
    assert r.numel() == 0


def test_int_candidates_draw_with_stream_round_times_world_plus_rank():
    streams = []
    for rank in (0, 1):
        m, eng, _ = wave(rank, 2, n=101)
        for rnd in (0, 1):
            eng.calls.clear()
            out = m.refine_collocation(40, 10, seed=9)
            kinds = [c[0] for c in eng.calls]
            assert kinds == ["sample_box", "score", "score", "keys", "select", "select"]
            assert eng.calls[0][1:] == (40, 9, rnd * 2 + rank, 0, tuple(RC.LB), tuple(RC.UB))
            assert eng.calls[3][3] == "mask" and eng.calls[3][2] == () and eng.calls[3][6:] == (9, rnd * 2 + rank)
            assert eng.calls[4][1:] == (40, 10, True)                                       # select_k ran on the keys of the 40 drawn points
            streams.append(eng.calls[0][3])
            P = SC.box64(9, rnd * 2 + rank, 0, 40, RC.LB, RC.UB).astype(np.float32)
            assert out["candidates"].shape == (out["replaced"], 3) and np.array_equal(out["candidates"].astype(np.float32), P[out["candidate_indices"]])
            lo, hi = m._shard(0, 101)
            if out["replaced"]:
                assert out["rows"].min() >= lo and out["rows"].max() < hi
                assert np.array_equal(np.stack(m._collo_host, axis=1)[out["rows"]], P[out["candidate_indices"]])
    assert sorted(streams) == [0, 1, 2, 3]
    m, eng, _ = wave()
    m.refine_collocation(10, 5, seed=1, stream=77, box=([1, 2, 3], [4, 5, 6]))
    assert eng.calls[-6][1:] == (10, 1, 77, 0, (1.0, 2.0, 3.0), (4.0, 5.0, 6.0)) and m._refine_round == 1
    with pytest.raises(ValueError):
        m.refine_collocation(10, 5, select="best")
    with pytest.raises(ValueError):
        m.refine_collocation(10, 5, exclude=[(1, 2, 3, 4)])                                 # a ball needs the four-column class
    with pytest.raises(ValueError):
        m.refine_collocation(10, 5, box=([0, 0], [1, 1]))


@pytest.mark.parametrize("select", ["top", "sample"])
def test_an_excluded_candidate_is_never_inserted(select):
    """50 candidates in a box of which a disc covers three quarters, K = 40 > the valid ones: select_k has to return excluded candidates too
    (key -inf); none goes in"""
    m, eng, Collo = wave()
    disc = (15.0, 15.0, 4.9)
    box = ([10.0, 10.0, 0.0], [20.0, 20.0, 20.0])
    P = SC.box64(4, 0, 0, 50, *box).astype(np.float32)
    valid = (P[:, 0] - np.float32(15)) ** 2 + (P[:, 1] - np.float32(15)) ** 2 > np.float32(4.9) ** 2
    assert 0 < valid.sum() < 40
    out = m.refine_collocation(50, 40, seed=4, box=box, exclude=[disc], select=select, c=0.5)
    assert eng.calls[-2][1:] == (50, 40, True) and eng.calls[-3][3] == ("mask" if select == "top" else "sample")
    assert 0 < out["replaced"] <= valid.sum() and valid[out["candidate_indices"]].all()
    want = Collo.copy()
    want[out["rows"]] = P[out["candidate_indices"]]
    assert np.array_equal(np.concatenate([m.x_c, m.y_c, m.t_c], axis=1), want) and m._n_collo == 120
    assert np.array_equal(np.stack([a.numpy() for a in m._collo], axis=1), want.astype(np.float32))


def test_array_candidates_make_the_calls_they_always_made():
    m, eng, _ = wave()
    cand = RC.points(50, seed=6)
    eng.calls.clear()
    out = m.refine_collocation(cand, 30)
    assert [c[0] for c in eng.calls] == ["score", "score", "select", "select"] and eng.calls[2][1:] == (50, 30, True)
    assert set(out) == {"replaced", "rows", "candidate_indices", "score_replaced_max", "score_inserted_min"}
    assert getattr(m, "_refine_round", 0) == 0
    eng.calls.clear()
    out = m.refine_collocation(cand, 30, exclude=[(15.0, 15.0, 5.0)])                        # an array with an excluded disc: keys, no draw
    assert [c[0] for c in eng.calls] == ["score", "score", "keys", "select", "select"] and "candidates" in out
    assert np.array_equal(out["candidates"], cand[out["candidate_indices"]])


def test_train_refines_behind_every_second_step():
    m, eng, _ = wave()
    seen = []
    real = m.refine_collocation
    m.refine_collocation = lambda *a, **kw: (seen.append((m.adam_t, a, dict(kw))), real(*a, **kw))[1]
    m.train(3, 1e-3, 2)
    assert seen == []                                                                      # refine=None: never
    t0 = m.adam_t
    m.train(3, 1e-3, 2, refine=dict(every=2, candidates=30, n_replace=5, seed=8, select="sample"))
    assert [s[0] - t0 for s in seen] == [2, 4, 6]                                          # counted over the whole call, across the blocks
    assert all(s[1] == (30, 5) and s[2] == {"seed": 8, "select": "sample"} for s in seen)
    assert sorted(c[3] for c in eng.calls if c[0] == "sample_box") == [0, 1, 2]            # one round each
    with pytest.raises(ValueError):
        RefineSchedule(m, dict(every=2, n_replace=5))
    with pytest.raises(ValueError):
        RefineSchedule(m, dict(every=0, candidates=10, n_replace=5))
    with pytest.raises(ValueError):
        RefineSchedule(m, dict(every=1, candidates=np.zeros((4, 3)), n_replace=5))
