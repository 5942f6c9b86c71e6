"""CPU model of the texture row of a side pixel when the batch kernel feeds it APPROXIMATE end quotients (cpuvox_amd/csrc/cvx_kernels.h: `tex_ends_approx`,
`tex_run<true>`, `tex_row_cheap`) against the reference's arithmetic on the correctly rounded quotients (DrawSegmentRayJob.cs:490-493, 524-531).

The model of tests/test_texture_row_model.py extended to the new inputs: every hardware reciprocal -- the two of the run's ends, which `recip_safe` then refines,
the run's own (1 / (boundsY - boundsX)) and the pixel's (1 / wux') -- is the correctly rounded reciprocal pushed one ulp either way, in every combination
(3^4 = 81), for both orders of the two ends.  No row that the widened bound calls certain may differ from the reference's row, and the widening may not cost the
renderer-shaped samples their certainty (the bar of the existing test).  The device test of the shipped instructions: tests/test_gpu_texture_row_inputs.py."""
import itertools

import numpy as np
import pytest

F = np.float32
E = 2.0 ** -24
K_ROUND = F(40.0 * E)  # tex_run: what the two arithmetics can differ by on the same inputs
K_INPUT = F(8.0 * E)  # tex_run<true>: what the approximate end quotients add


def _fma(a, b, c):
    # a * b is exact in float64 (two 24-bit significands); one rounding to float64 and one to float32 stand for the fused operation
    # (a double rounding can differ from the true fma by an ulp in rare cases: inside the error the bound assumes for every operation anyway)
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)


def _rcp(x, ulps):
    """v_rcp_f32 as the derivation assumes it: within one ulp of 1 / x.  The reciprocal of a zero is the instruction's exact result (an infinity, which has no
    neighbour one ulp away): a run whose span boundsY - boundsX rounds to zero must stay what it is on the device, a run without a certain pixel."""
    with np.errstate(all="ignore"):
        r0 = (F(1.0) / x).astype(F)
    r = r0
    for _ in range(abs(ulps)):
        r = np.nextafter(r, F(np.inf) if ulps > 0 else F(-np.inf)).astype(F)
    return np.where(np.isfinite(r0), r, r0).astype(F)


def _div_safe(x):
    a = np.abs(x)
    return (a >= F(2.0 ** -30)) & (a <= F(2.0 ** 30))


def _recip_safe(d, ulps):
    """recip_safe: the hardware reciprocal (here: off by `ulps`) and one Newton step."""
    r = _rcp(d, ulps)
    e = _fma(-d, r, np.ones_like(d))
    return _fma(e, r, r)


def exact_ends(zb, zt, ua):
    """uvA = (1, uA) / bottom.z, uvB = (1, 0) / top.z as the reference divides them."""
    with np.errstate(all="ignore"):
        return (F(1.0) / zb).astype(F), (ua / zb).astype(F), (F(1.0) / zt).astype(F), (F(0.0) / zt).astype(F)


def approx_ends(zb, zt, ua, kb, kt, at_the_limit=False):
    """tex_ends_approx where both depths are in the safe range and uA is a run length, the reference's divisions elsewhere (the kernel's `!ordinary` lanes).
    at_the_limit: not recip_safe's result but the worst the header's bound allows it to be, the correctly rounded quotient's neighbour on the side of (kb, kt)."""
    ax, ay, bx, by = exact_ends(zb, zt, ua)
    with np.errstate(all="ignore"):
        rb, rt = _recip_safe(zb, kb), _recip_safe(zt, kt)
        if at_the_limit:
            rb, rt = _rcp(zb, kb), _rcp(zt, kt)
        ok = _div_safe(zb) & _div_safe(zt) & (ua >= F(1.0)) & (ua <= F(65535.0))  # (uA is a run's length)
        return np.where(ok, rb, ax), np.where(ok, (ua * rb).astype(F), ay), np.where(ok, rt, bx), by


def exact_row(y, bx, by, uvax, uvbx, uvay, uvby):
    with np.errstate(all="ignore"):
        l = ((y - bx) / (by - bx)).astype(F)
        wux = (uvax + (l * (uvbx - uvax).astype(F)).astype(F)).astype(F)
        wuy = (uvay + (l * (uvby - uvay).astype(F)).astype(F)).astype(F)
        return (wuy / wux).astype(F)


def cheap_row_wide(y, bx, by, uvax, uvbx, uvay, uvby, k1, k2):
    """tex_run<true> + tex_row_cheap<true>, operation for operation."""
    with np.errstate(all="ignore"):
        d = (by - bx).astype(F)
        rd = np.where(np.abs(d) <= F(2.0 ** 100), _rcp(d, k1), F(np.nan)).astype(F)
        a1, a2 = (uvbx - uvax).astype(F), (uvby - uvay).astype(F)
        s1 = (np.abs(uvax) + np.abs(uvbx)).astype(F)
        kk = F(K_ROUND + K_INPUT)
        a1s = _fma(K_INPUT, s1, (K_ROUND * np.abs(a1)).astype(F))
        bxs = _fma(kk, np.abs(uvax), F(2.0 ** -140))
        n = (y - bx).astype(F)
        lq = (n * rd).astype(F)
        wx, wy = _fma(lq, a1, uvax), _fma(lq, a2, uvay)
        r = _rcp(wx, k2)
        uq = (wy * r).astype(F)
        sx = _fma(np.abs(lq), a1s, bxs)
        sxy = _fma(kk, _fma(np.abs(lq), np.abs(a2), np.abs(uvay)), sx)  # Sy + Sx, Sy = 48 e (|uvA.y| + |l'| |a2|)
        t = _fma(np.abs(uq), sx, sxy)
        bound = _fma(t, np.abs(r), _fma(np.abs(wx), F(2.0 ** -110), (F(2.0 ** -21) * np.abs(uq)).astype(F)))
        certain = np.abs((uq - np.rint(uq)).astype(F)) > bound
    return uq, certain


def _near_integer_run_lengths(rng, y, bx, span, zb, zt, ua):
    """a third of the samples: the run length chosen so that the row lands next to an integer for this pixel (where the floor is decided)"""
    n = len(y)
    t = np.clip((y - bx) / span, 0.0, 1.0)
    target = np.rint(rng.uniform(1, 60, n)) + rng.uniform(-1, 1, n) * np.exp(rng.uniform(np.log(1e-8), np.log(1e-3), n))
    wx = 1.0 / zb + t * (1.0 / zt - 1.0 / zb)
    near = rng.random(n) < 0.33
    return np.where(near & (t < 0.98), target * wx * zb / np.maximum(1.0 - t, 1e-9), ua)


def samples(family, seed, n, near_integer=True):
    """{y, boundsX, boundsY, bottom.z, top.z, uA} as float32; boundsX <= boundsY wherever they are ordered (the kernel's swap is the caller's `swap`)."""
    rng = np.random.default_rng(seed)
    if family in ("renderer", "level", "deep"):
        span = np.exp(rng.uniform(np.log(0.01), np.log(3000.0), n))
        bx = rng.uniform(-200.0, 2300.0, n)
        by = bx + span
        y = np.rint(rng.uniform(bx, by)).clip(-2, 16385)  # the pixels of a run: rint(boundsX) .. rint(boundsY)
        zb = np.exp(rng.uniform(np.log(0.5), np.log(6000.0), n))
        zt = zb * np.exp(rng.uniform(-1.5, 1.5, n))
        if family == "level":  # a level camera: both ends at (nearly) the same depth, uvB.x - uvA.x cancels
            zt = zb * (1.0 + rng.uniform(-1e-4, 1e-4, n) * rng.integers(0, 2, n))
        if family == "deep":  # ends far apart in depth
            zt = zb * np.exp(rng.uniform(-4.0, 4.0, n))
        ua = np.rint(np.exp(rng.uniform(0.0, np.log(600.0), n)))
        if near_integer:
            ua = _near_integer_run_lengths(rng, y, bx, span, zb, zt, ua)
    elif family == "extreme":  # depths to 0.06, spans to 1e-4, y one pixel outside the bounds: |l'| in the thousands
        span = np.exp(rng.uniform(np.log(1e-4), np.log(3000.0), n))
        bx = rng.uniform(-200.0, 2300.0, n)
        by = bx + span
        y = np.rint(rng.uniform(bx - 1.0, by + 1.0)).clip(-2, 16385)
        zb = np.exp(rng.uniform(np.log(0.06), np.log(6000.0), n))
        zt = zb * np.exp(rng.uniform(-4.0, 4.0, n) * rng.integers(0, 2, n))
        ua = np.rint(np.exp(rng.uniform(0.0, np.log(65535.0), n)))
        ua = _near_integer_run_lengths(rng, y, bx, span, zb, zt, ua)
    elif family == "soup":  # any float at all in every operand (non-finite, denormal, either sign)
        bits = rng.integers(0, 2 ** 32, (5, n), dtype=np.uint64).astype(np.uint32).view(F)
        bx, by, zb, zt, ua = bits
        y = rng.integers(-2, 16386, n).astype(np.float64)
        # half of the depths inside the range where the kernel takes the short form (any sign), run lengths as the world has them
        pick = rng.random(n) < 0.5
        zb = np.where(pick, np.exp(rng.uniform(np.log(2.0 ** -30), np.log(2.0 ** 30), n)) * rng.choice([-1.0, 1.0], n), zb)
        zt = np.where(pick, np.exp(rng.uniform(np.log(2.0 ** -30), np.log(2.0 ** 30), n)) * rng.choice([-1.0, 1.0], n), zt)
        ua = np.where(rng.random(n) < 0.7, np.rint(np.exp(rng.uniform(0.0, np.log(65535.0), n))), ua)
        near = rng.random(n) < 0.5  # half of the bounds near the pixel, so that some rows are certain
        with np.errstate(all="ignore"):
            bx = np.where(near, y - rng.uniform(-1.0, 40.0, n), bx)
            by = np.where(near, bx + np.exp(rng.uniform(np.log(1e-4), np.log(3000.0), n)) * rng.choice([-1.0, 1.0], n), by)
    else:
        raise ValueError(family)
    with np.errstate(all="ignore"):
        return tuple(np.asarray(v).astype(F) for v in (y, bx, by, zb, zt, ua))


def swapped(ends, swap):
    """:496-499: the end with the smaller bound comes first; `swap` = the top end is that one."""
    ax, ay, bx, by = ends
    return (bx, by, ax, ay) if swap else (ax, ay, bx, by)


def check(family, seed, n, swap, near_integer=True, at_the_limit=False):
    """Every combination of reciprocals off by -1, 0, +1 ulp: asserts that no certain row differs, returns the share of rows certain in all of them."""
    y, bx, by, zb, zt, ua = samples(family, seed, n, near_integer)
    ax, ay, bxx, byy = swapped(exact_ends(zb, zt, ua), swap)
    exact = exact_row(y, bx, by, ax, bxx, ay, byy)
    certain_all = np.ones(n, dtype=bool)
    for kb, kt in itertools.product((-1, 0, 1), repeat=2):
        qax, qay, qbx, qby = swapped(approx_ends(zb, zt, ua, kb, kt, at_the_limit), swap)
        for k1, k2 in itertools.product((-1, 0, 1), repeat=2):
            uq, certain = cheap_row_wide(y, bx, by, qax, qbx, qay, qby, k1, k2)
            with np.errstate(all="ignore"):
                wrong = certain & (np.floor(uq) != np.floor(exact))
            assert not wrong.any(), f"{family}, reciprocals off by ({kb}, {kt}, {k1}, {k2}) ulp: {wrong.sum()} certain rows differ, first at {np.flatnonzero(wrong)[0]}"
            certain_all &= certain
    return certain_all.mean()


def test_refined_reciprocal_is_within_one_ulp_of_the_quotient():
    """The bound the header states for `recip_safe`'s result: the correctly rounded 1 / d or one of its two neighbours, whichever way the hardware's
    reciprocal was off; and the product uA * r within 3.01 * 2^-24 of uA / d."""
    rng = np.random.default_rng(7)
    n = 400_000
    d = (np.exp(rng.uniform(np.log(2.0 ** -30), np.log(2.0 ** 30), n)) * rng.choice([-1.0, 1.0], n)).astype(F)
    d[: 2 ** 16] = np.linspace(1.0, 2.0, 2 ** 16, dtype=F)  # one binade densely, its edges included
    ua = np.rint(np.exp(rng.uniform(0.0, np.log(65535.0), n))).astype(F)
    q = (F(1.0) / d).astype(F)
    lo, hi = np.nextafter(q, F(-np.inf)), np.nextafter(q, F(np.inf))
    true = 1.0 / d.astype(np.float64)
    for k in (-1, 0, 1):
        r = _recip_safe(d, k)
        assert ((r == q) | (r == lo) | (r == hi)).all()
        assert (np.abs(r.astype(np.float64) - true) <= 2.0 ** -23 * np.abs(true)).all()
        p = (ua * r).astype(F)
        assert (np.abs(p.astype(np.float64) - ua.astype(np.float64) * true) <= 3.01 * E * np.abs(ua * true)).all()


FAMILIES = [("renderer", 1), ("level", 2), ("deep", 3), ("extreme", 4), ("soup", 5)]


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("family,seed", FAMILIES)
def test_certain_rows_equal_the_reference_rows(family, seed, swap):
    """recip_safe's own results for a hardware reciprocal off by an ulp either way (the correctly rounded quotient nearly always: the widening is rarely needed)."""
    check(family, seed, 200_000, swap)


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("family,seed", FAMILIES)
def test_certain_rows_equal_the_reference_rows_with_ends_at_the_limit_of_the_bound(family, seed, swap):
    """The end reciprocals as far off as the header's bound allows recip_safe's result to be: a neighbour of the correctly rounded quotient, on either side, in every
    sample.  (Without the new terms -- K_INPUT = 0 -- thousands of these rows are wrong: the level camera's, where a1 cancels, first.)"""
    check(family, seed + 10, 200_000, swap, at_the_limit=True)


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("family,seed", [("renderer", 21), ("deep", 23), ("level", 22)])
def test_renderer_shaped_rows_stay_certain(family, seed, swap):
    """Run lengths as they come (no row placed next to an integer on purpose).  The bar of the device test of the narrow form (0.97) for depths in [0.5, 6000] and
    spans >= 0.01, both orders; the level camera, where the new terms are the whole of the per-pixel part of Sx, is printed: 0.963 against 0.984 for the narrow
    form on exact ends."""
    share = check(family, seed, 200_000, swap, near_integer=False)
    print(f"{family} swap={swap}: certain in every one of the 81 combinations: {share:.4f}")
    if family != "level":
        assert share > 0.97
