"""CPU checks of tests/loss_edges.py and of the power of tests/test_loss_edges_gpu.py: the pinned-ratio reference is plain ext_loss
autograd away from the boundaries; the tables hold what they promise (exact ties, every rung of every ladder under numpy's float32
exp); and a float32 restatement of the kernel's rule, judged exactly as the GPU test judges the kernel, passes every case as it stands
and fails a NAMED case for every defect switched on in it.  The tables are the GPU module's own.  Nothing here touches a device.

Left out of DEFECTS because no case could tell them from the correct rule (loss_edges' docstring): a min() tie weight of 1 / 0 or 0 / 1,
and lo / hi formed as 1.0f -/+ (float)clip (asserted equal below)."""
import numpy as np
import pytest

import loss_edges as E
import test_loss_edges_gpu as gpu_cases
from ppo_reference import ext_loss

f32 = np.float32


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


_TABLES = {}


def _observed(torch, A, act):
    """The table of (A, act) observed with numpy's float32 exp in the device's place: (cases, ratios, missing, disagree, reference)."""
    if (A, act) not in _TABLES:
        cases = E.with_twins(E.table(A, act))
        cases, r, missing, disagree = E.complete(cases, E.host_observation(cases))
        _TABLES[A, act] = (cases, r, missing, disagree, E.reference(torch, cases, r))
    return _TABLES[A, act]


def _tiny_policy(A):
    """Offsets of a D = 1, H = 1, L = 1 policy: the smallest packed buffer ext_loss accepts."""
    return {"W0": (0, (1, 1)), "b0": (1, (1,)), "Wpi": (2, (A, 1)), "bpi": (2 + A, (A,)), "Wv": (2 + 2 * A, (1, 1)), "bv": (3 + 2 * A, (1,))}


@pytest.mark.parametrize("A,act", gpu_cases.TABLE_KEYS)
def test_pinned_reference_is_ext_loss_autograd_away_from_the_boundaries(torch, A, act):
    """ext_loss gets the constants the kernel holds (f32 roundings) but forms 1 -/+ clip itself, so pg is compared where the clamp is idle."""
    cases = [c for c in E.table(A, act) if c.ladder is None]
    offsets = _tiny_policy(A)
    r = np.array([np.exp(E.lp64(c.bpi)[c.act] - c.logp) for c in cases])
    for c, x in zip(cases, r):                                                  # away: no ratio within 1e-4 of a bound
        lo, hi, _ = E.bounds32(c.cfg.clip)
        assert min(abs(x - float(lo)), abs(x - float(hi))) > 1e-4, c.name
    ref = E.reference(torch, cases, r)
    for i, c in enumerate(cases):
        p = torch.zeros(4 + 2 * A, dtype=torch.float64)
        p[:2] = 0.5
        p[2 + A: 2 + 2 * A] = torch.tensor(c.bpi, dtype=torch.float64)
        p[3 + 2 * A] = c.bv
        p.requires_grad_(True)
        t = lambda v: torch.tensor([v], dtype=torch.float64)  # noqa: E731
        kw = dict(clip=float(f32(c.cfg.clip)), vf_coef=float(f32(c.cfg.vf_coef)), ent_coef=float(f32(c.cfg.ent_coef)),
                  vf_clip=float(f32(c.cfg.vf_clip)), kl_coef=float(f32(c.cfg.kl_coef)))
        out = ext_loss(torch, p, offsets, 1, "tanh", torch.tensor([[0.3]], dtype=torch.float64), torch.tensor([c.act]), t(c.logp), t(c.adv),
                       t(c.ret), t(c.val), torch.tensor([c.lpo[:A]], dtype=torch.float64), **kw)
        out[0].backward()
        got = np.append(p.grad[2 + A: 2 + 2 * A].numpy(), p.grad[3 + 2 * A].item())
        want = np.append(ref["dz"][i], ref["dv"][i])
        assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want) + 1e-300), (c.name, got, want)
        assert float(p.grad[:2].abs().max()) == 0.0                              # (the head weights are zero: nothing reaches the trunk)
        lo, hi, _ = E.bounds32(c.cfg.clip)
        for k, (mine, theirs) in enumerate(zip(ref["terms"][i], [float(o.detach()) for o in out[1:6]])):
            if k == 0 and not float(lo) < r[i] < float(hi):
                continue
            if k == 4 and not c.cfg.kl_coef > 0:
                assert mine == 0.0
                continue
            assert abs(mine - theirs) <= 1e-12 * abs(theirs) + 1e-300, (c.name, k, mine, theirs)


@pytest.mark.parametrize("A", [2, 4])
def test_the_minibatch_reference_is_the_mean_of_the_per_sample_references(torch, A):
    """pinned_minibatch_grad over a whole table at one parameter set (zero head weights) against reference() case by case: the head
    biases' gradient is the mean of dz / dv, the head weights' the mean of dz[j] * h[k], the trunk's zero."""
    Dn, H = 7, 16
    shapes = [("W0", (H, Dn)), ("b0", (H,)), ("Wpi", (A, H)), ("bpi", (A,)), ("Wv", (1, H)), ("bv", (1,))]
    offsets, P = {}, 0
    for k, s in shapes:
        offsets[k] = (P, s)
        P += int(np.prod(s))
    g = torch.Generator().manual_seed(A)
    p = torch.rand(P, generator=g) - 0.5
    for k in ("Wpi", "Wv"):
        p[offsets[k][0]: offsets[k][0] + int(np.prod(offsets[k][1]))] = 0.0
    (ob, _), (ov, _), (ow, _) = offsets["bpi"], offsets["bv"], offsets["Wpi"]
    p[ob: ob + A] = torch.tensor(E.distributions(A, 0)["p95"])
    p[ov] = 0.0
    cases = E.with_twins(E.table(A, 0, rungs=4))
    n = len(cases)
    x = torch.rand((n, Dn), generator=g)
    group = [c._replace(bpi=tuple(float(v) for v in p[ob: ob + A]), bv=0.0, cfg=E.GROUP_CFG) for c in cases]
    r = np.array([E.host_heads(c.bpi, c.act, c.logp)[2] for c in group], dtype=f32)
    whole = E.pinned_minibatch_grad(torch, p, offsets, 1, "tanh", x, cases, r, E.GROUP_CFG, torch.float64).numpy()
    per = E.reference(torch, group, r)
    h = torch.tanh(x.double() @ p[: H * Dn].double().view(H, Dn).T + p[H * Dn: H * Dn + H].double()).numpy()
    close = lambda a, b: np.all(np.abs(a - b) <= 1e-12 * np.abs(b).max())  # noqa: E731
    assert close(whole[ob: ob + A], per["dz"].mean(0)) and close(whole[ov], per["dv"].mean())
    assert close(whole[ow: ow + A * H].reshape(A, H), per["dz"].T @ h / n) and not whole[: H * Dn + H].any()


# defect -> the label of a case that must fail under it
CATCHES = {"ratio_clamp_exclusive": "ratio/clip0.2/hi/at/An=+1", "vclamp_exclusive": "value/c0.0625/d=c/tie_inside/ret=0",
           "min_tie_00": "ratio/clip0.2/far=1/An=+1", "min_tie_11": "ratio/clip0.1/far=1/An=-1",
           "max_tie_10": "value/c0.05/d=c+/tie_clamped", "max_tie_01": "value/c0.5/d=-c-/tie_clamped",
           "vclamp_mask_from_max": "value/c0.5/d=c-/tie_inside/ret=0", "kl_without_sum": "kl/unnormalised_half",
           "clipfrac_ge": "ratio/clip0.3/lo/at/An=+1"}


def _rule_results(cases, r, defect):
    out = [E.sample_rule(c, x, defect) for c, x in zip(cases, r)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


@pytest.mark.parametrize("A,act", gpu_cases.TABLE_KEYS)
def test_the_correct_rule_passes_and_every_defect_fails_a_named_case(torch, A, act):
    cases, r, missing, disagree, ref = _observed(torch, A, act)
    assert not missing and not disagree
    fails, worst = E.judge(cases, r, ref, *_rule_results(cases, r, None))
    assert not fails, fails[:5]
    assert worst <= 2.5e-6, worst
    assert set(CATCHES) == set(E.DEFECTS)
    for defect in E.DEFECTS:
        fails, _ = E.judge(cases, r, ref, *_rule_results(cases, r, defect))
        assert CATCHES[defect] in {f[0] for f in fails}, (defect, sorted({f[0] for f in fails})[:10])
        if defect != "clipfrac_ge":                                              # a wrong branch is half of S or more, not a rounding
            i = [E.label(c, x) for c, x in zip(cases, r)].index(CATCHES[defect])
            dl, dv, _ = E.sample_rule(cases[i], r[i], defect)
            _, rel = E.within_bound(np.append(dl, dv), np.append(ref["dz"][i], ref["dv"][i]), np.append(ref["Sz"][i], ref["Sv"][i]))
            assert rel.max() >= 0.25, (defect, rel)


def test_defects_left_out_cannot_be_told_apart():
    for clip in E.CLIPS:
        lo, hi, c = E.bounds32(clip)
        assert lo == f32(f32(1.0) - c) and hi == f32(f32(1.0) + c), clip


def test_the_clip_fraction_is_not_the_clamp():
    """The finding of loss_edges' docstring: fabsf(r - 1) > (float)clip against r outside [lo, hi]."""
    counted = {clip: tuple(float(E.clip_fraction_bit(b, clip)) for b in E.bounds32(clip)[:2]) for clip in E.CLIPS}
    assert counted == {0.1: (1.0, 1.0), 0.2: (0.0, 1.0), 0.3: (0.0, 0.0)}
    differ = {(clip, which) for clip in E.CLIPS for which, b in zip(("lo", "hi"), E.bounds32(clip)[:2])
              if E.clip_fraction_bit(b, clip) != E.clip_fraction_bit(b, clip, "clipfrac_ge")}
    assert differ == {(0.3, "lo")}
    for clip in E.CLIPS:                                                        # one float outside either bound is always counted
        for which, b in zip(("lo", "hi"), E.bounds32(clip)[:2]):
            t = E.rung_targets(clip, which)
            assert E.clip_fraction_bit(t["below" if which == "lo" else "above"], clip) == 1.0


@pytest.mark.parametrize("A", [2, 3, 4])
def test_every_tie_that_claims_exactness_is_exact_in_float32(A):
    seen = {"tie_clamped": 0, "tie_inside": 0, "l1>l2": 0, "l2>l1": 0}
    for c in E.table(A, 0, rungs=1):
        if not c.name.startswith("value"):
            continue
        rec = E.checked_value_case(c.name.split("/", 2)[2], f32(c.bv), f32(c.val), f32(c.ret), c.cfg.vf_clip)   # (also run at table())
        for k in seen:
            if k in c.name:
                seen[k] += 1
                assert rec["rel"] == {"l1>l2": "l1", "l2>l1": "l2"}.get(k, "tie"), c.name
                assert k != "tie_clamped" or (not rec["vin"] and rec["l1"] > 0), c.name
        assert f32(c.bv) == c.bv and f32(c.val) == c.val and f32(c.ret) == c.ret                        # the batch holds these floats
    assert seen["tie_clamped"] >= 4 * len(E.VF_CLIPS) and all(seen.values()), seen


@pytest.mark.parametrize("A,act", gpu_cases.TABLE_KEYS)
def test_the_ladders_reach_every_rung_under_numpys_float32_exp(A, act):
    cases = [c for c in E.table(A, act) if c.ladder is not None and c.adv == 1.0]
    ratios = {}
    for c in cases:
        ratios.setdefault(c.ladder[:2], []).append(E.host_heads(c.bpi, c.act, c.logp)[2])
    assert len(ratios) == 2 * len(E.CLIPS)
    for (clip, which), rs in ratios.items():
        targets = E.rung_targets(clip, which)
        assert all(t in rs for t in targets.values()), (clip, which)


def test_step_f32_walks_consecutive_floats():
    for x in (f32(0.3), f32(-0.3), f32(1.0), f32(-2.0 ** -126)):
        assert E.step_f32(x, 1) == np.nextafter(x, f32(np.inf)) and E.step_f32(x, -1) == np.nextafter(x, f32(-np.inf))
        assert E.step_f32(E.step_f32(x, 37), -37) == x


def test_clip_coef_at_its_boundary():
    for norm in (f32(0.0123), f32(3.5), f32(1e-3)):
        m0 = f32(norm + f32(1e-6))
        assert E.clip_coef(m0, norm) == 1.0 and E.clip_coef(np.nextafter(m0, f32(np.inf)), norm) == 1.0
        assert E.clip_coef(np.nextafter(m0, f32(0.0)), norm) < 1.0
    assert E.clip_coef(1e-30, 0.0) == f32(f32(1e-30) / f32(1e-6)) and E.clip_coef(1.0, 0.0) == 1.0
