"""The PPO loss's per-sample decisions at their boundaries: case tables, an f64 autograd reference of ONE sample's loss as a function of
(logits, value), and numpy float32 restatements of what is a single f32 operation chain in ppo_grad_body.  No device, no pytest:
tests/test_loss_edges.py runs the tables against the restatement (with defects switched on) on the host, tests/test_loss_edges_gpu.py
against the kernels.

How one sample becomes observable.  A policy whose head weights Wpi and Wv are zero has logits == bpi and value == bv in every kernel
that computes a forward, so with a minibatch of ONE sample (M = 1, the divisor is (float)1) the gradient's bpi entries are the kernel's
own dl[j], its bv entry is dv, and the stats row holds that sample's terms.  Everything else a case needs is a batch row.

The ratio goes through the device's expf, which the host cannot predict to the bit, so it is READ: with An = +1 the pg stat is
-min(r, hi), with An = -1 it is max(r, lo) (`observe`).  Every (bpi, act, logp) key of a table has both twins.  The reference is then
evaluated with the ratio pinned to the observed float, ratio = r_obs * exp(lp - lp.detach()): its value is r_obs exactly, its derivative
the true one; the decision and the derivative stay the reference's (torch.min / torch.clamp / torch.max: 0.5 / 0.5 on ties, gradient 1
at a clamp's bounds).  A ladder of f32 logp_old values around lp[act] - log(bound) walks the ratio across each bound in steps of less
than a third of an ulp; `rung_cases` then adds the An = +0, -0, 2^-120 cases at one rung each of {bound-, bound, bound+}.

The tolerance is |mine - ref| <= 1e-5 * S + 1e-30 per component, S = the sum of the magnitudes of the component's addends: per loss
term T with g = dT/dlogp and G = sum(g), the softmax backward's g[j] and -p[j]*G; for the value, T's own derivative.  (With An = 2^-120
the gradient is ~1e-36, under the 1e-30 floor: those cases check the stats and that nothing but a tiny number comes out.)

Findings, computed by the float32 restatement (test_loss_edges.py asserts each):
  * the clip fraction counts fabsf(r - 1) > (float)clip, which is NOT "r outside [lo, hi]": with clip = 0.2, r == lo is not counted
    (1 - lo = 0.19999999 < 0.2f) but r == hi is (hi - 1 = 0.20000005 > 0.2f) although the clamp passes the gradient there; with clip = 0.1
    both bounds are counted; with clip = 0.3 neither is (hi - 1 = 0.29999995 < 0.3f), and 1 - lo == 0.3f exactly, so r == lo is the one
    ratio of these tables at which `>` and `>=` differ.  One float outside either bound is always counted.
  * (float)(1.0 - clip) == 1.0f - (float)clip and (float)(1.0 + clip) == 1.0f + (float)clip for clip in (0.1, 0.2, 0.3): forming the
    bounds in f32 cannot be told apart from the header's rule on these tables, so that defect is not in DEFECTS.
  * min(s1, s2) ties only where both sides carry the same derivative (r inside the clamp) or none (An == 0), so a tie weight of 1 / 0 or
    0 / 1 gives the gradient of 0.5 / 0.5 on every case a table could hold; what CAN be told apart is a pair of weights that does not add
    up to 1 (two strict comparisons and no tie branch: 0 / 0; two inclusive ones: 1 / 1).  DEFECTS holds those instead.
  * max(l1, l2) ties with the clamp ACTIVE do tell 1 / 0 and 0 / 1 from 0.5 / 0.5 (the l2 side is blocked there)."""
from collections import namedtuple

import numpy as np

f32 = np.float32
F1, F0 = f32(1.0), f32(0.0)
TINY_ADV = 2.0 ** -120
ADVS = (("+1", 1.0), ("-1", -1.0), ("+0", 0.0), ("-0", -0.0), ("2^-120", TINY_ADV))
CLIPS = (0.1, 0.2, 0.3)
VF_CLIPS = (0.0625, 0.05, 0.5)
LADDER_RUNGS = 32           # each side of the centre (the ladder may be widened to 64)
BOUND_REL, BOUND_ABS = 1e-5, 1e-30

Cfg = namedtuple("Cfg", "clip vf_clip vf_coef ent_coef kl_coef")
Case = namedtuple("Case", "name A bpi bv act logp adv ret val lpo cfg ladder")   # ladder: None or (clip, "lo" / "hi", rung)
GROUP_CFG = Cfg(0.2, 0.0625, 0.5, 0.01, 1.0)    # every case's batch row in one minibatch


def ratio_cfg(clip):
    return Cfg(clip, 0.0, 0.0, 0.0, 0.0)


def bounds32(clip):
    """(lo, hi, clip) as the library rounds them: 1 -/+ clip formed in double, then f32."""
    return f32(1.0 - clip), f32(1.0 + clip), f32(clip)


def step_f32(x, n):
    """The float32 n representable values above x (below for n < 0)."""
    i = np.array([x], dtype=f32).view(np.int32).astype(np.int64)[0]
    i = i if i >= 0 else -(i & 0x7FFFFFFF)          # an integer that orders the floats
    i += n
    i = i if i >= 0 else (-i) | 0x80000000
    return np.array([i & 0xFFFFFFFF], dtype=np.uint32).view(f32)[0]


# ------------------------------------------------------------------------------------------------------------------------------------
# numpy float32 restatements
# ------------------------------------------------------------------------------------------------------------------------------------
def host_heads(bpi, act, logp):
    """ppo_grad_body's softmax and ratio in numpy float32 (the device's expf / logf may differ in the last bit): (lp, p, ratio)."""
    lg = np.asarray(bpi, dtype=f32)
    m = lg.max()
    se = F0
    with np.errstate(under="ignore"):
        for x in lg:
            se = f32(se + np.exp(f32(x - m)))
        lse = f32(m + np.log(se))
        lp = (lg - lse).astype(f32)
        p = np.exp(lp).astype(f32)
        ratio = np.exp(f32(lp[act] - f32(logp)))
    return lp, p, f32(ratio)


def clip_fraction_bit(ratio, clip, defect=None):
    c = f32(clip)
    a = np.abs(f32(f32(ratio) - F1))
    return F1 if (a >= c if defect == "clipfrac_ge" else a > c) else F0


def value_rule(v, v_old, ret, vf_clip, defect=None):
    """The value clip's f32 chain: d, err, errc, l1, l2, vl = max(l1, l2), the weights, the clamp's mask, gv = d VL / d v."""
    v, vo, ret, c = f32(v), f32(v_old), f32(ret), f32(vf_clip)
    err = f32(v - ret)
    l1 = f32(err * err)
    if not c > 0:
        return dict(d=None, err=err, errc=None, l1=l1, l2=None, vl=l1, gv=f32(f32(2.0) * err), vin=None, rel=None)
    d = f32(v - vo)
    errc = f32(f32(vo + min(max(d, -c), c)) - ret)
    l2 = f32(errc * errc)
    tie = l1 == l2
    t1, t2 = {"max_tie_10": (1.0, 0.0), "max_tie_01": (0.0, 1.0)}.get(defect, (0.5, 0.5))
    w1 = f32(1.0 if l1 > l2 else (t1 if tie else 0.0))
    w2 = f32(1.0 if l2 > l1 else (t2 if tie else 0.0))
    if defect == "vclamp_exclusive":
        vin = -c < d < c
    elif defect == "vclamp_mask_from_max":
        vin = bool(l2 > l1)
    else:
        vin = -c <= d <= c
    gv = f32(f32(w1 * f32(f32(2.0) * err)) + (f32(w2 * f32(f32(2.0) * errc)) if vin else F0))
    return dict(d=d, err=err, errc=errc, l1=l1, l2=l2, vl=max(l1, l2), gv=gv, vin=vin, rel="tie" if tie else ("l1" if l1 > l2 else "l2"))


def clip_coef(max_grad_norm, norm):
    """ppo_clip_body's coefficient on an f32 norm: min(1, max_grad_norm / (norm + 1e-6f))."""
    return min(F1, f32(f32(max_grad_norm) / f32(f32(norm) + f32(1e-6))))


DEFECTS = ("ratio_clamp_exclusive", "vclamp_exclusive", "min_tie_00", "min_tie_11", "max_tie_10", "max_tie_01", "vclamp_mask_from_max",
           "kl_without_sum", "clipfrac_ge")


def sample_rule(case, ratio, defect=None):
    """ppo_grad_body's loss and gradient of one sample (M = 1) in numpy float32, given the ratio: (dl [A], dv, [pg, VL, entropy, clip
    fraction, KL]).  defect: one of DEFECTS, the rule a subtly wrong kernel would follow."""
    cfg, A = case.cfg, case.A
    lo, hi, _ = bounds32(cfg.clip)
    lp, p, _ = host_heads(case.bpi, case.act, case.logp)
    ratio, An = f32(ratio), f32(case.adv)
    with np.errstate(under="ignore", invalid="ignore", over="ignore"):
        ent = F0
        for j in range(A):
            ent = f32(ent - f32(p[j] * lp[j]))
        s1, s2 = f32(ratio * An), f32(min(max(ratio, lo), hi) * An)
        t = {"min_tie_00": 0.0, "min_tie_11": 1.0}.get(defect, 0.5)
        gmin = f32(-1.0)
        g1 = gmin if s1 < s2 else (f32(t) * gmin if s1 == s2 else F0)
        g2 = gmin if s2 < s1 else (f32(t) * gmin if s1 == s2 else F0)
        inside = (lo < ratio < hi) if defect == "ratio_clamp_exclusive" else (lo <= ratio <= hi)
        gr = f32(f32(g1 * An) + (f32(g2 * An) if inside else F0))
        glpa, gent = f32(gr * ratio), f32(-f32(cfg.ent_coef))
        dl = np.zeros(A, dtype=f32)
        for j in range(A):
            dl[j] = f32(f32(glpa * f32((F1 if j == case.act else F0) - p[j])) + f32(gent * f32(-p[j] * f32(lp[j] + ent))))
        kl = F0
        if cfg.kl_coef > 0:
            lpo = np.asarray(case.lpo[:A], dtype=f32)
            po = np.exp(lpo).astype(f32)
            spo = F0
            for j in range(A):
                spo = f32(spo + po[j])
                kl = f32(kl + f32(po[j] * f32(lpo[j] - lp[j])))
            if defect == "kl_without_sum":
                spo = F1
            for j in range(A):
                dl[j] = f32(dl[j] + f32(f32(cfg.kl_coef) * f32(f32(p[j] * spo) - po[j])))
        vr = value_rule(case.bv, case.val, case.ret, cfg.vf_clip, defect)
        dv = f32(f32(cfg.vf_coef) * vr["gv"])
        terms = [f32(-min(s1, s2)), vr["vl"], ent, clip_fraction_bit(ratio, cfg.clip, defect), kl]
    return dl, dv, terms


# ------------------------------------------------------------------------------------------------------------------------------------
# the case tables
# ------------------------------------------------------------------------------------------------------------------------------------
def lp64(bpi):
    z = np.asarray(bpi, dtype=f32).astype(np.float64)
    return z - (z.max() + np.log(np.exp(z - z.max()).sum()))


def distributions(A, act):
    """name -> head biases [A] f32: 0.95 on the acted action; uniform; one logit (not the acted one) 20, then 120, below the rest."""
    other = (act + 1) % A
    out = {"p95": [0.0] * A, "uniform": [0.0] * A, "low20": [0.0] * A, "low120": [0.0] * A}
    out["p95"][act] = float(np.log(0.95 * (A - 1) / 0.05))
    out["low20"][other], out["low120"][other] = -20.0, -120.0
    return {k: tuple(float(f32(x)) for x in v) for k, v in out.items()}


def _logp_for(bpi, act, ratio):
    return f32(lp64(bpi)[act] - np.log(float(ratio)))


def _ladder(bpi, act, clip, which, rungs):
    """[(rung, logp_old)]: f32 values `stride` floats apart around lp[act] - log(bound), the stride such that one rung moves the ratio
    by at most a third of its ulp (1 = consecutive floats)."""
    lo, hi, _ = bounds32(clip)
    bound = lo if which == "lo" else hi
    centre = _logp_for(bpi, act, bound)
    per_float = float(bound) * float(np.spacing(np.abs(centre)))
    stride = max(1, int(float(np.spacing(bound)) / (3.0 * per_float)))
    return [(k, step_f32(centre, k * stride)) for k in range(-rungs, rungs + 1)]


def _value_cases(A, c64):
    """(name, v, v_old, ret) with every number chosen so that d, err and errc are exact in f32 (`checked_value_case` asserts it)."""
    c = f32(c64)
    dn, up = np.nextafter(c, F0), np.nextafter(c, f32(np.inf))
    out = []
    for name, d in (("-c+", -dn), ("-c", -c), ("-0", f32(-0.0)), ("+0", F0), ("c-", dn), ("c", c)):   # inside: v_old = 0, l1 == l2 always
        rets = [("tie_inside/ret=0", F0), ("tie_inside/ret=2d", f32(2.0) * d), ("v==ret", d)]
        if d == 0:
            rets = [("tie_inside/ret=+.25", f32(0.25)), ("tie_inside/ret=-.25", f32(-0.25)), ("v==ret", d)]
        out += [("d=%s/%s" % (name, r), d, F0, ret) for r, ret in rets]
    outside = [("-c-", f32(c - up), c), ("c+", f32(up - c), -c), ("far-", f32(-1.0), c), ("far+", F1, -c)]   # v_old = -+c: the clamped value is 0
    for name, v, vo in outside:
        out += [("d=%s/%s" % (name, r), v, vo, ret) for r, ret in
                (("l1>l2", -v), ("l2>l1", f32(2.0) * v), ("tie_clamped", f32(0.5) * v), ("v==ret", v))]
    if float(c) == c64:                                                    # a dyadic clip: also v_old = 0, the clamped value +-c
        for sign in (-1.0, 1.0):
            v, vc = f32(sign * 3.0) * c, f32(sign) * c
            out += [("d=far%s/vo=0/%s" % ("+" if sign > 0 else "-", r), v, F0, ret) for r, ret in
                    (("l1>l2", -vc), ("l2>l1", f32(5.0) * vc), ("tie_clamped", f32(2.0) * vc), ("v==ret", v))]
    return out


def checked_value_case(name, v, vo, ret, c64):
    """Assert that the f32 chain of a value case is exact and sits where its name says; returns value_rule's record."""
    r = value_rule(v, vo, ret, c64)
    c = float(f32(c64))
    v64, vo64, ret64 = float(v), float(vo), float(ret)
    d64 = v64 - vo64
    assert float(r["err"]) == v64 - ret64 and float(r["errc"]) == vo64 + min(max(d64, -c), c) - ret64, name
    if "far" not in name:
        assert float(r["d"]) == d64, name
    rung, rel = name.split("/")[0][2:], name.split("/")[-1]
    want_d = {"-c-": d64 < -c, "-c": d64 == -c, "-c+": -c < d64 < 0, "-0": d64 == 0 and np.signbit(r["d"]), "+0": d64 == 0 and not np.signbit(r["d"]),
              "c-": 0 < d64 < c, "c": d64 == c, "c+": d64 > c, "far-": d64 < -c, "far+": d64 > c}[rung]
    assert want_d, name
    dn, up = float(np.nextafter(f32(c), F0)), float(np.nextafter(f32(c), f32(np.inf)))
    assert abs(d64) == {"-c-": up, "-c+": dn, "c-": dn, "c+": up}.get(rung, abs(d64)), name    # the floats NEXT to the clamp's bounds
    l1, l2 = (v64 - ret64) ** 2, float(r["errc"]) ** 2
    exact_rel = "tie" if l1 == l2 else ("l1" if l1 > l2 else "l2")
    assert r["rel"] == exact_rel, name                                           # f32's comparison is the exact one
    want_rel = {"l1>l2": "l1", "l2>l1": "l2", "tie_clamped": "tie", "v==ret": None}.get(rel, "tie")
    assert want_rel is None or r["rel"] == want_rel, name
    assert r["vin"] == (rung in ("-c", "-c+", "-0", "+0", "c-", "c")), name
    return r


def _peaked(A, at, height=5.0):
    z = [0.0] * A
    z[at] = height
    return z


def _lpo(vals, A, pad=0.0):
    return tuple(float(f32(x)) for x in vals) + (pad,) * (4 - A)


def table(A, act, rungs=LADDER_RUNGS):
    """The static cases of an (n_actions, acted action) pair; `with_twins` completes it."""
    dists = distributions(A, act)
    p95, zero_lpo = dists["p95"], (0.0,) * 4
    lp95 = float(lp64(p95)[act])
    assert -0.125 < lp95 < 0
    cases = []

    def add(name, bpi, logp, adv, cfg, bv=0.0, ret=0.0, val=0.0, lpo=zero_lpo, ladder=None):
        cases.append(Case(name, A, tuple(bpi), float(bv), act, float(logp), float(adv), float(ret), float(val), tuple(lpo), cfg, ladder))

    # the ratio: ladders across each bound (An = +-1: they are also the observations), and ratios far inside and outside
    for clip in CLIPS:
        for which in ("lo", "hi"):
            for k, logp in _ladder(p95, act, clip, which, rungs):
                for an, adv in ADVS[:2]:
                    add("ladder/clip%g/%s/k=%+d/An=%s" % (clip, which, k, an), p95, logp, adv, ratio_cfg(clip), ladder=(clip, which, k))
        for r in (0.5, 1.0, 2.0):
            for an, adv in ADVS:
                add("ratio/clip%g/far=%g/An=%s" % (clip, r, an), p95, _logp_for(p95, act, r), adv, ratio_cfg(clip))
    # the other distributions: ratios near the bounds, the entropy term on
    for dname in ("uniform", "low20", "low120"):
        for r in (0.7992, 0.8008, 1.0, 1.1988, 1.2012):
            for an, adv in ADVS[:2]:
                add("dist/%s/r=%g/An=%s" % (dname, r, an), dists[dname], _logp_for(dists[dname], act, r), adv, Cfg(0.2, 0.0, 0.5, 0.01, 0.0),
                    bv=0.25, ret=-0.5)
    # the value clip
    uni = dists["uniform"]
    for c64 in VF_CLIPS:
        for name, v, vo, ret in _value_cases(A, c64):
            checked_value_case(name, v, vo, ret, c64)
            add("value/c%g/%s" % (c64, name), uni, _logp_for(uni, act, 1.0), 0.0, Cfg(0.2, c64, 0.5, 0.0, 0.0), bv=v, ret=ret, val=vo)
    # the KL term (advantage 0: its gradient alone)
    cur95, curu = lp64(p95), lp64(uni)
    peaked = lp64(_peaked(A, (act + 1) % A))
    under = [-100.0] + [float(np.log(1.0 / (A - 1)))] * (A - 1)
    nan = float("nan")
    kl = [("same", p95, _lpo(cur95, A), 1.0), ("old_peaked_new_flat", uni, _lpo(peaked, A), 1.0),
          ("old_flat_new_peaked", _peaked(A, (act + 1) % A), _lpo(curu, A), 1.0),
          ("unnormalised_half", p95, _lpo(cur95 + np.log(0.5), A), 0.5), ("old_logp_-100", uni, _lpo(under, A), 1.0)]
    if A < 4:
        kl.append(("garbage_padding", uni, _lpo(peaked, A, pad=nan), 1.0))
    for name, bpi, lpo, coef in kl:
        bpi = tuple(float(f32(x)) for x in bpi)
        add("kl/%s" % name, bpi, _logp_for(bpi, act, 1.0), 0.0, Cfg(0.2, 0.0, 0.0, 0.0, coef), lpo=lpo)
    return cases


def key_of(case):
    return (case.bpi, case.act, case.logp)


def with_twins(cases):
    """`cases` plus an An = +1 and an An = -1 case for every (bpi, act, logp) key that lacks one: every ratio can be read."""
    have = {(key_of(c), c.adv) for c in cases if c.adv in (1.0, -1.0)}
    out, seen = list(cases), set()
    for c in cases:
        for an, adv in ADVS[:2]:
            if (key_of(c), adv) not in have and (key_of(c), adv) not in seen:
                seen.add((key_of(c), adv))
                out.append(c._replace(name="twin/%s/An=%s" % (c.name, an), adv=adv, cfg=ratio_cfg(0.2), ladder=None))
    return out


def observe(cases, pg):
    """The ratio of every case, read from the pg stats of its key's twins: -pg(An = +1) = min(r, hi), pg(An = -1) = max(r, lo).
    Returns (r_obs f32 [n], the keys at which both twins reveal the ratio and disagree)."""
    lo_of, hi_of = {}, {}
    for c, s in zip(cases, pg):
        lo, hi, _ = bounds32(c.cfg.clip)
        if c.adv == 1.0:
            hi_of.setdefault(key_of(c), []).append((f32(-s), hi))
        elif c.adv == -1.0:
            lo_of.setdefault(key_of(c), []).append((f32(s), lo))
    r_of, disagree = {}, []
    for k in hi_of:
        seen = {float(a) for a, hi in hi_of[k] if a < hi} | {float(b) for b, lo in lo_of[k] if b > lo}
        assert seen, k                                              # (hi > lo: one twin always reveals)
        if len(seen) > 1:
            disagree.append(k)
        r_of[k] = f32(min(seen))
    return np.array([r_of[key_of(c)] for c in cases], dtype=f32), disagree


def host_observation(cases):
    """What `observe` would read if the device's expf were numpy's: the pg stat of every case."""
    return [sample_rule(c, host_heads(c.bpi, c.act, c.logp)[2])[2][0] for c in cases]


RUNG_NAMES = ("below", "at", "above")


def rung_targets(clip, which):
    lo, hi, _ = bounds32(clip)
    b = lo if which == "lo" else hi
    return dict(zip(RUNG_NAMES, (np.nextafter(b, F0), b, np.nextafter(b, f32(np.inf)))))


def label(case, r):
    """The name that says which decision a case sits on, given its observed ratio."""
    if case.ladder is None:
        return case.name
    clip, which, _ = case.ladder
    where = [n for n, t in rung_targets(clip, which).items() if t == r]
    return "ratio/clip%g/%s/%s/An=%s" % (clip, which, where[0] if where else "off", case.name.split("An=")[1])


def rung_cases(cases, r_obs):
    """(new cases, missing): for every ladder and each of {bound-, bound, bound+} the first rung whose observed ratio is that float,
    with An = +0, -0 and 2^-120 (its An = +-1 cases are the ladder's own); missing lists the (clip, bound, rung) no ladder rung reached."""
    first, new, missing = {}, [], []
    for c, r in zip(cases, r_obs):
        if c.ladder is not None and c.adv == 1.0:
            for where, t in rung_targets(*c.ladder[:2]).items():
                if t == r:
                    first.setdefault(c.ladder[:2] + (where,), c)
    for clip in CLIPS:
        for which in ("lo", "hi"):
            for where in RUNG_NAMES:
                c = first.get((clip, which, where))
                if c is None:
                    missing.append((clip, which, where))
                    continue
                new += [c._replace(name="ladder/clip%g/%s/k=%+d/An=%s" % (clip, which, c.ladder[2], an), adv=adv) for an, adv in ADVS[2:]]
    return new, missing


# ------------------------------------------------------------------------------------------------------------------------------------
# the f64 autograd reference
# ------------------------------------------------------------------------------------------------------------------------------------
def _pinned(torch, r):
    return lambda lp: r * torch.exp(lp - lp.detach())


def _rounded(cfg):
    """The constants as the kernel holds them (f32 roundings, include/shipsim.h), widened to python floats."""
    lo, hi, clip = bounds32(cfg.clip)
    return dict(clip=float(clip), vf_clip=float(f32(cfg.vf_clip)), bounds=(float(lo), float(hi))), \
        [1.0, float(f32(cfg.vf_coef)), float(f32(cfg.ent_coef)), float(f32(cfg.kl_coef))]


def reference(torch, cases, r_obs, dtype=None):
    """Autograd of every case's M = 1 loss as a function of (logits z, value v), the ratio pinned to r_obs: a dict of numpy f64 arrays
    dz [n, A], dv [n], Sz [n, A], Sv [n] (the sums of the magnitudes of the addends) and terms [n, 5] (pg, VL, entropy, clip fraction,
    KL).  The cases share A; they are evaluated in one batch per configuration."""
    from ppo_reference import ext_sample_terms
    dtype = dtype or torch.float64
    n, A = len(cases), cases[0].A
    out = dict(dz=np.zeros((n, A)), dv=np.zeros(n), Sz=np.zeros((n, A)), Sv=np.zeros(n), terms=np.zeros((n, 5)))
    groups = {}
    for i, c in enumerate(cases):
        assert c.A == A
        groups.setdefault(c.cfg, []).append(i)
    for cfg, ids in groups.items():
        col = lambda f: torch.tensor([f(cases[i]) for i in ids], dtype=dtype)  # noqa: E731
        z = col(lambda c: c.bpi).requires_grad_(True)
        v = col(lambda c: c.bv).requires_grad_(True)
        a = torch.tensor([cases[i].act for i in ids], dtype=torch.long)
        r = torch.tensor(np.asarray(r_obs, dtype=np.float64)[ids], dtype=dtype)
        kw, coefs = _rounded(cfg)
        lpa = torch.log_softmax(z, -1)
        smin, vls, plp, kls, clipped, _ = ext_sample_terms(torch, lpa, v, a, None, col(lambda c: c.adv), col(lambda c: c.ret), col(lambda c: c.val),
                                                            col(lambda c: c.lpo[:A]), ratio_of=_pinned(torch, r), **kw)
        if not cfg.kl_coef > 0:
            kls = torch.zeros_like(kls)
        pieces = [-smin, vls, plp, kls]                                         # (- ent_coef * entropy = + ent_coef * sum(p * logp))
        total = sum(w * t.sum() for w, t in zip(coefs, pieces))
        dz, dv = torch.autograd.grad(total, [z, v], retain_graph=True, allow_unused=True)
        # the addends: per term, d/d logp (the softmax backward then adds g[j] and -p[j] * sum(g)) and d/d v
        p = lpa.detach().exp()
        Sz, Sv = torch.zeros_like(p), torch.zeros_like(v)
        for w, t in zip(coefs, pieces):
            if w == 0.0 or not t.requires_grad:
                continue
            g, gv = torch.autograd.grad(w * t.sum(), [lpa, v], retain_graph=True, allow_unused=True)
            if g is not None:
                Sz = Sz + g.abs() + p * g.sum(-1, keepdim=True).abs()
            if gv is not None:
                Sv = Sv + gv.abs()
        out["dz"][ids] = (torch.zeros_like(z) if dz is None else dz).double().numpy()
        out["dv"][ids] = (torch.zeros_like(v) if dv is None else dv).double().numpy()
        out["Sz"][ids], out["Sv"][ids] = Sz.double().numpy(), Sv.double().numpy()
        terms = [-smin, vls, -plp, clipped.to(dtype), kls]
        out["terms"][ids] = torch.stack([t.detach().double() for t in terms], -1).numpy()
    return out


def within_bound(mine, ref, S):
    """|mine - ref| <= 1e-5 * S + 1e-30, elementwise; also returns |mine - ref| / S where S > 1e-20 (else 0)."""
    mine, ref, S = (np.asarray(x, dtype=np.float64) for x in (mine, ref, S))
    err = np.abs(mine - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(S > 1e-20, err / S, 0.0)
    return ~(err > BOUND_REL * S + BOUND_ABS), rel


def complete(cases, pg):
    """A table after its observation: (cases + rung_cases, the ratio of each, the rungs no ladder reached, the keys whose twins
    disagree).  pg: the pg stat of every case of `cases` (which holds every key's twins)."""
    r, disagree = observe(cases, pg)
    new, missing = rung_cases(cases, r)
    r_of = {key_of(c): x for c, x in zip(cases, r)}
    return cases + new, np.concatenate([r, np.array([r_of[key_of(c)] for c in new], dtype=f32)]), missing, disagree


def judge(cases, r_obs, ref, dl, dv, stats):
    """What a kernel's M = 1 results must satisfy, case by case: dl [n][A] and dv [n] within the bound of the f64 reference `ref`
    (reference()'s dict), and bit for bit: the clip-fraction stat = the restatement's; stats[1] = its max(l1, l2); pg = -hi for An = +1
    above hi and +lo for An = -1 below lo; KL = +0.0 with the term off.  stats: [n][>= 4] (pg, VL, entropy, clip fraction[, KL]).
    Returns (the failures as (label, what, got, want), the largest |mine - ref| / S)."""
    fails, worst = [], 0.0
    for i, (c, r) in enumerate(zip(cases, r_obs)):
        lo, hi, _ = bounds32(c.cfg.clip)
        name = label(c, r)
        ok, rel = within_bound(np.append(dl[i], dv[i]), np.append(ref["dz"][i], ref["dv"][i]), np.append(ref["Sz"][i], ref["Sv"][i]))
        worst = max(worst, float(rel.max()))
        if not ok.all():
            fails.append((name, "gradient", [float(x) for x in np.append(dl[i], dv[i])], [float(x) for x in np.append(ref["dz"][i], ref["dv"][i])]))
        st = [f32(x) for x in stats[i]]
        want = [("clip fraction", st[3], clip_fraction_bit(r, c.cfg.clip)), ("VL", st[1], value_rule(c.bv, c.val, c.ret, c.cfg.vf_clip)["vl"])]
        if c.adv == 1.0 and r > hi:
            want.append(("pg", st[0], -hi))
        if c.adv == -1.0 and r < lo:
            want.append(("pg", st[0], lo))
        if len(st) > 4 and not c.cfg.kl_coef > 0:
            want.append(("KL", st[4], F0))
        for what, got, w in want:
            if not (got == w and np.signbit(got) == np.signbit(w)):
                fails.append((name, what, float(got), float(w)))
    return fails, worst


def pinned_minibatch_grad(torch, params, offsets, L, activation, x, cases, r_obs, cfg, dtype):
    """Autograd of the MEAN loss of the cases' batch rows (all under `cfg`) at packed parameters `params`, every ratio pinned: the
    gradient in `dtype`, on params' device."""
    from ppo_reference import ext_sample_terms, forward
    dev, A = params.device, cases[0].A
    col = lambda f: torch.tensor([f(c) for c in cases], dtype=dtype, device=dev)  # noqa: E731
    p = params.detach().to(dtype).clone().requires_grad_(True)
    logits, v = forward(torch, p, offsets, L, activation, x.to(dtype))
    kw, coefs = _rounded(cfg)
    r = torch.tensor(np.asarray(r_obs, dtype=np.float64), dtype=dtype, device=dev)
    a = torch.tensor([c.act for c in cases], dtype=torch.long, device=dev)
    smin, vls, plp, kls, _, _ = ext_sample_terms(torch, torch.log_softmax(logits, -1), v, a, None, col(lambda c: c.adv), col(lambda c: c.ret), col(lambda c: c.val), col(lambda c: c.lpo[:A]),
                                                 ratio_of=_pinned(torch, r), **kw)
    loss = coefs[0] * (-smin).mean() + coefs[1] * vls.mean() + coefs[2] * plp.mean() + coefs[3] * kls.mean()
    loss.backward()
    return p.grad.detach()
