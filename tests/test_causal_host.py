"""CPU tests of the host side of causal sampling (no library): residual_profile, resample_collocation, refine_collocation(causal=True) and
train(causal=...) of the wave classes on a stand-in engine -- tests/test_refine_sampling_host.SamplingEngine plus binned_sums, causal_cdf and
sample_box(t_cdf=...) from the numpy references of tests/_causal_cases.py."""
import numpy as np
import pytest
import torch

from pinn_elastodynamics_amd.causal import CausalSchedule, PROBE_STREAM
from pinn_elastodynamics_amd.elastic_wave import DeepHPM, DeepHPMConfined
from tests import _causal_cases as CC
from tests import _refine_cases as RC
from tests import _sample_cases as SC
from tests.test_refine_host import LAYERS, sets
from tests.test_refine_sampling_host import SamplingEngine

DISC = (15.0, 15.0, 6.0)
PROFILE = ["sample_box", "score", "keys", "binned"]
REDRAW = ["cdf", "sample_box", "keys", "select"]


class CausalEngine(SamplingEngine):
    """SamplingEngine with HipEngine's binned_sums / causal_cdf / sample_box(t_cdf=...): the numpy references"""

    def sample_box(self, n, lo, hi, seed, stream=0, first=0, t_cdf=None):
        if t_cdf is None:
            return super().sample_box(n, lo, hi, seed, stream, first)
        self.calls.append(("sample_box", int(n), int(seed), int(stream), int(first), tuple(lo), tuple(hi), t_cdf))
        P = CC.draw_reference(seed, stream, first, n, lo, hi, t_cdf.numpy())[0]
        return tuple(torch.from_numpy(np.ascontiguousarray(P[:, k])) for k in range(P.shape[1]))

    def binned_sums(self, value, coord, lo, hi, n_bins, out=None):
        self.calls.append(("binned", value.numel(), float(lo), float(hi), int(n_bins)))
        sums, counts, _ = CC.binned_reference(value.numpy(), coord.numpy(), lo, hi, n_bins)
        return torch.from_numpy(np.stack([sums, counts]))

    def causal_cdf(self, binned, eps, floor=0.0):
        self.calls.append(("cdf", float(eps), float(floor)))
        _, _, w, _, cdf32 = CC.cdf_reference(binned.numpy(), eps, floor)
        return torch.from_numpy(w), torch.from_numpy(cdf32)


def wave(rank=0, world=1, n=120):
    Collo, SRC, IC, UP = sets(n)
    eng = CausalEngine(LAYERS)
    if world == 1:
        return DeepHPM(Collo, SRC, IC, UP, LAYERS, RC.LB, RC.UB, engine=eng, verbose=False, seed=3), eng, Collo
    return DeepHPMConfined(Collo.copy(), SRC, IC, UP, None, LAYERS, None, None, RC.LB, RC.UB, engine=eng, verbose=False, seed=3,
                           shard_as=(rank, world)), eng, Collo


def kinds(eng):
    return [c[0] for c in eng.calls]


def in_disc(P, disc=DISC):
    return (P[:, 0] - disc[0]) ** 2 + (P[:, 1] - disc[1]) ** 2 <= disc[2] ** 2


def test_the_reference_sampler_meets_the_share_bar_alone():
    """the seed and the table of the 65536-point share tests (emulator, GPU): the numpy sampler itself is within 5 binomial sigma in every bin"""
    tab = CC.general_table(16)
    _, b, _ = CC.draw_reference(CC.SHARE_SEED, CC.SHARE_STREAM, 0, CC.SHARE_N, RC.LB, RC.UB, tab)
    sig, empty = CC.share_errors(b, tab)
    assert (np.diff(tab) > 0).all() and tab[0] == 0 and tab[-1] == 1 and np.diff(tab).max() > 50 * np.diff(tab).min()
    assert (sig <= 5.0).all() and empty.size == 0, sig
    P, b, t64 = CC.draw_reference(1, 0, 0, 4096, RC.LB, RC.UB, CC.GAP_TABLE)
    assert set(np.unique(b)) == {1, 3, 4} and (np.abs(P[:, 2] - t64) <= CC.t_bound(RC.LB[2], RC.UB[2])).all()


def test_residual_profile_makes_four_calls_on_the_probe_stream():
    profiles = []
    for rank in (0, 1):
        m, eng, _ = wave(rank, 2, n=101)
        m._refine_round = 5
        eng.calls.clear()
        prof, counts = m.residual_profile(8, 300, exclude=[DISC], seed=9)
        assert kinds(eng) == PROFILE
        assert eng.calls[0][1:] == (300, 9, PROBE_STREAM | 5, 0, tuple(RC.LB), tuple(RC.UB))      # the same points on both ranks
        assert eng.calls[1][1] == 300 and eng.calls[1][3] is False                                # not the packed weights of an older step
        assert eng.calls[2][2:4] == ((DISC,), "mask") and eng.calls[3][1:] == (300, RC.LB[2], RC.UB[2], 8)
        assert prof.shape == counts.shape == (8,) and m._refine_round == 5
        P = SC.box64(9, PROBE_STREAM | 5, 0, 300, RC.LB, RC.UB).astype(np.float32)
        assert counts.sum() == (~in_disc(P, np.float32(DISC))).sum() < 300 and (prof >= 0).all() and prof.max() > 0
        profiles.append((prof, counts))
    assert all(np.array_equal(a, b) for a, b in zip(*profiles))
    with pytest.raises(ValueError):
        m.residual_profile(0, 300)
    with pytest.raises(ValueError):
        m.residual_profile(65, 300)
    with pytest.raises(ValueError):
        m.residual_profile(8, 300, exclude=[(1, 2, 3, 4)])


def test_resample_redraws_this_ranks_rows_only():
    tables, streams = [], []
    for rank in (0, 1):
        m, eng, Collo = wave(rank, 2, n=101)
        for rnd in (0, 1):
            eng.calls.clear()
            before = np.stack(m._collo_host, axis=1).copy()
            out = m.resample_collocation(dict(bins=8, eps=2.0, candidates=400, exclude=[DISC], seed=9))
            assert kinds(eng) == PROFILE + REDRAW and set(out) == {"redrawn", "kept", "w", "cdf", "profile", "counts"}
            lo, hi = m._shard(0, 101)
            n_draw = (hi - lo) + (hi - lo) // 8 + 64
            assert eng.calls[0][3] == PROBE_STREAM | rnd and eng.calls[5][1:4] == (n_draw, 9, rnd * 2 + rank)
            assert eng.calls[5][7] is m._causal_cdf and eng.calls[6][2:4] == ((DISC,), "mask") and eng.calls[7][1:] == (n_draw, hi - lo, True)
            assert eng.calls[4][1] == pytest.approx(2.0 / m._causal_ref) and eng.calls[4][2] == 0.0
            assert out["redrawn"] == hi - lo and out["kept"] == 0 and m._refine_round == rnd + 1
            assert out["w"].shape == (8,) and out["w"][0] == 1.0 and out["cdf"].shape == (9,) and np.array_equal(out["cdf"], m._causal_cdf.numpy())
            P = CC.draw_reference(9, rnd * 2 + rank, 0, n_draw, RC.LB, RC.UB, out["cdf"])[0]
            want = before.copy()
            want[lo:hi] = P[~in_disc(P, np.float32(DISC))][:hi - lo]                              # the first N_shard valid points, in order
            assert np.array_equal(np.stack(m._collo_host, axis=1), want) and not in_disc(want[lo:hi]).any()
            assert np.array_equal(np.concatenate([m.x_c, m.y_c, m.t_c], axis=1).astype(np.float32), want)
            assert np.array_equal(np.stack([a.numpy() for a in m._collo], axis=1), want[lo:hi]) and m._n_collo == 101
            streams.append(eng.calls[5][3])
            if rnd == 0:
                tables.append((out["cdf"], out["profile"], out["counts"], m._causal_ref))
        assert np.array_equal(Collo, sets(101)[0])                                                # the caller's array is not written
    assert sorted(streams) == [0, 1, 2, 3]
    assert all(np.array_equal(a, b) for a, b in zip(*tables))                                     # the same table on both ranks, no collective
    ref = tables[0][3]
    assert ref == pytest.approx((tables[0][1] * tables[0][2]).sum() / tables[0][2].sum())


def test_single_process_bookkeeping_and_a_float_ref():
    m, eng, Collo = wave()
    out = m.resample_collocation(dict(bins=4, eps=1.0, candidates=200, ref=0.5, floor=0.1))
    assert ("cdf", 2.0, 0.1) in eng.calls and not hasattr(m, "_causal_ref") and out["redrawn"] == 120
    got = np.stack([a.numpy() for a in m._collo_full], axis=1)
    assert np.array_equal(got, np.stack(m._collo_host, axis=1)) and np.array_equal(got, np.concatenate([m.x_c, m.y_c, m.t_c], axis=1).astype(np.float32))
    assert m._collo_cache == {} and np.isfinite(m.getloss()[0])
    m.resample_collocation(dict(bins=4, eps=5.0, candidates=200, floor=0.1))                      # ref="first": eps in units of the mean score
    shares = np.bincount(CC.bin_rule(m._collo_full[2].numpy(), RC.LB[2], RC.UB[2], 4), minlength=4)
    assert shares[0] > shares[3]                                                                  # early times hold more of the rows


def test_a_short_draw_keeps_exactly_the_deficit_of_old_rows():
    """a disc over most of the box and no slack: fewer valid points than rows -- the first m rows are drawn again, the rest keep their bits"""
    m, eng, _ = wave()
    big = (15.0, 15.0, 14.0)
    before = np.stack(m._collo_host, axis=1).copy()
    out = m.resample_collocation(dict(bins=4, eps=1.0, candidates=200, exclude=[big], seed=2, slack=0))
    P = CC.draw_reference(2, 0, 0, 120, RC.LB, RC.UB, out["cdf"])[0]
    valid = ~in_disc(P, np.float32(big))
    k = int(valid.sum())
    assert 0 < k < 120 and out["redrawn"] == k and out["kept"] == 120 - k
    after = np.stack(m._collo_host, axis=1)
    assert np.array_equal(after[:k], P[valid]) and np.array_equal(after[k:], before[k:])
    assert np.array_equal(np.stack([a.numpy() for a in m._collo], axis=1), after)
    assert kinds(eng).count("sample_box") == 2                                                    # no loop, no fallback draw


def test_refine_with_causal_draws_from_the_table():
    m, eng, _ = wave()
    with pytest.raises(ValueError):
        m.refine_collocation(40, 10, causal=True)                                                 # no table yet
    m.resample_collocation(dict(bins=8, eps=1.0, candidates=200))
    with pytest.raises(ValueError):
        m.refine_collocation(RC.points(40, seed=6), 10, causal=True)                              # an array is not drawn
    eng.calls.clear()
    out = m.refine_collocation(40, 10, seed=4, causal=True)
    assert kinds(eng) == ["sample_box", "score", "score", "keys", "select", "select"]
    assert eng.calls[0][1:4] == (40, 4, 1) and eng.calls[0][7] is m._causal_cdf                   # round 1: the redraw was round 0
    P = CC.draw_reference(4, 1, 0, 40, RC.LB, RC.UB, m._causal_cdf.numpy())[0]
    assert np.array_equal(out["candidates"].astype(np.float32), P[out["candidate_indices"]])
    eng.calls.clear()
    m.refine_collocation(40, 10, seed=4)
    assert len(eng.calls[0]) == 7                                                                 # causal=False: the call without a table


def test_train_without_causal_makes_the_calls_it_always_made():
    logs = []
    for kw in ({}, {"causal": None}):
        m, eng, _ = wave()
        m.train(3, 1e-3, 2, **kw)
        logs.append(list(eng.calls))
    assert logs[0] == logs[1] and not {"binned", "cdf", "sample_box"} & {c[0] for c in logs[0]}
    m, eng, _ = wave(0, 2)
    assert len(m.train(2, 1e-3, 1, causal=None)) == 3                                             # the confined class takes the keyword too


def test_train_triggers_behind_every_second_step_in_front_of_refinement():
    m, eng, _ = wave()
    eng.calls.clear()
    m.train(4, 1e-3, 1, causal=dict(every=2, bins=8, eps=1.0, candidates=200, seed=1), refine=dict(every=2, candidates=30, n_replace=5, seed=1))
    k = [c for c in kinds(eng) if c in ("binned", "cdf", "select", "wave")]
    per_trigger = ["binned", "cdf", "select", "select", "select"]                                 # the profile, the table, the redraw; refinement's two
    assert k == ["wave", "wave"] + per_trigger + ["wave", "wave"] + per_trigger
    boxes = [c for c in eng.calls if c[0] == "sample_box"]
    assert [c[3] for c in boxes] == [PROBE_STREAM | 0, 0, 1, PROBE_STREAM | 2, 2, 3] and m._refine_round == 4


def test_a_first_train_call_redraws_at_every_trigger():
    """ref="first" (the default) on a fresh model: the FIRST trigger takes the scale from its own profile and redraws, so the steps behind it
    already train on a causal set -- one block of 6 steps with every=2 is three profiles, three tables and three redraws, none thrown away;
    the scale is fetched once and holds for the later triggers and the next call"""
    m, eng, _ = wave()
    eng.calls.clear()
    before = np.stack(m._collo_host, axis=1).copy()
    m.train(6, 1e-3, 1, causal=dict(every=2, bins=8, eps=1.5, candidates=200))
    k = [c for c in kinds(eng) if c in ("binned", "cdf", "select", "wave")]
    assert k == ["wave", "wave", "binned", "cdf", "select"] * 3 and m._refine_round == 3
    probes = [c for c in eng.calls if c[0] == "sample_box" and c[3] & PROBE_STREAM]
    draws = [c for c in eng.calls if c[0] == "sample_box" and not c[3] & PROBE_STREAM]
    assert [c[3] for c in probes] == [PROBE_STREAM | r for r in range(3)] and [c[3] for c in draws] == [0, 1, 2]
    # the scale is the mean score of the FIRST profile's probe points, and every table of the call is made with it
    i = kinds(eng).index("binned")
    first = eng.calls[i - 3]
    assert first[0] == "sample_box" and first[1:4] == (200, 0, PROBE_STREAM)
    ref = m._causal_ref
    assert ref > 0 and [c[1] for c in eng.calls if c[0] == "cdf"] == [pytest.approx(1.5 / ref)] * 3
    # the rows behind the first trigger are the draw of round 0 from the first table -- not the rows the model was built with
    assert not np.array_equal(np.stack(m._collo_host, axis=1), before)
    eng.calls.clear()
    m.train(2, 1e-3, 1, causal=dict(every=2, bins=8, eps=1.5, candidates=200))
    assert m._causal_ref == ref and [c[1] for c in eng.calls if c[0] == "cdf"] == [pytest.approx(1.5 / ref)] and m._refine_round == 4


def test_bad_entries_raise():
    m, _, _ = wave()
    good = dict(every=2, bins=8, eps=1.0, candidates=100)
    CausalSchedule(m, good, ("x_c", "y_c", "t_c"))
    for bad in (dict(good, bins=0), dict(good, bins=65), dict(good, eps=-1.0), dict(good, eps=float("nan")), dict(good, floor=-0.1),
                dict(good, candidates=0), dict(good, candidates=np.zeros((4, 3))), dict(good, every=0), dict(good, ref="last"),
                dict(good, ref=-1.0), dict(good, colour=1), dict(good, exclude=[(1, 2)]), {k: v for k, v in good.items() if k != "every"},
                {k: v for k, v in good.items() if k != "bins"}):
        with pytest.raises(ValueError):
            m.train(1, 1e-3, 1, causal=bad)
    with pytest.raises(ValueError):
        m.resample_collocation(dict(bins=8, eps=1.0))
    with pytest.raises(ValueError):
        m.resample_collocation(dict(good))                                                        # `every` belongs to train
