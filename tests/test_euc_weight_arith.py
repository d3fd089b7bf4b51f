"""CPU restatement of the arithmetic of edge_w<TSPGPU_EUC_2D, F32R> (csrc/tspgpu.hip: the weight every kernel uses for the
headline kind): x = (float)sq, the one-ulp v_sqrt_f32 root r, its two bit neighbours rm / rp, the two FMA residuals
x - rm*r and x - rp*r, the two selects that leave the correctly rounded f32 root c, then (int)((double)c + 0.5) -- and, F32R,
(int)(c + 0.5f) in f32.  Checked against oracle/cpu_ref.c's formula (int)((double)sqrtf((float)sq) + 0.5) for every root the
hardware may return: v_sqrt_f32 is specified to one ulp, so the correctly rounded root AND its two neighbours must all lead
to the same weight.  The residuals are single FMAs on the device (one rounding: the sign of the exact value); here the
products are formed in f64, where rm*r and rp*r (48 bits) are exact and the subtraction keeps the sign.

Samples: integer and fractional coordinate differences up to the largest box whose diagonal stays below 2^27 (the top of the
int32 cells), sq = 0, sq at and one f32 step either side of (k + 0.5)^2 (where the rounding to an integer flips) and of k^2
for k < 2^27, every power of two up to 2^53 with two f32 neighbours on each side (the binade edges of the root); the F32R form
only on roots below 4.0e6, the guard of tspgpu_build_costs, the largest such root included."""
import numpy as np

F32R_BOUND = 4.0e6                 # tspgpu_build_costs: f32r = EUC_2D && cost_bound < 4.0e6
BOX = 94906265                     # the largest integer side s with s * sqrt 2 < 2^27


def f32_step(v, steps):
    """the f32 array v moved by `steps` units in the last place (towards +-inf)"""
    v = v.astype(np.float32)
    for _ in range(abs(steps)):
        v = np.nextafter(v, np.float32(np.inf if steps > 0 else -np.inf))
    return v


def weight(sq, ulps, f32r):
    """edge_w<TSPGPU_EUC_2D, f32r> from the f64 sum of squares, with the hardware root moved by `ulps` units in the last place"""
    x = sq.astype(np.float32)                                    # (float)sq: round to nearest even
    r = f32_step(np.sqrt(x), ulps)                               # numpy's f32 sqrt is correctly rounded
    ri = r.view(np.int32)
    rm, rp = (ri - 1).view(np.float32), (ri + 1).view(np.float32)           # x = 0: rm is a NaN, rp the smallest denormal
    X, R = x.astype(np.float64), r.astype(np.float64)
    with np.errstate(invalid="ignore"):
        em = X - rm.astype(np.float64) * R                       # fmaf(-rm, r, x)
        ep = X - rp.astype(np.float64) * R                       # fmaf(-rp, r, x)
        c = np.where(0.0 >= em, rm, r)                           # a NaN residual compares false: c = r
    c = np.where(0.0 < ep, rp, c).astype(np.float32)
    if f32r:
        return (c + np.float32(0.5)).astype(np.float32).astype(np.int64)
    return (c.astype(np.float64) + 0.5).astype(np.int64)


def want(sq):
    """oracle/cpu_ref.c: (int)((double)sqrtf((float)sq) + 0.5)"""
    return (np.sqrt(sq.astype(np.float32)).astype(np.float64) + 0.5).astype(np.int64)


def samples():
    rs = np.random.RandomState(3)
    parts = [np.zeros(1)]
    dx, dy = rs.randint(-BOX, BOX + 1, 600000).astype(np.float64), rs.randint(-BOX, BOX + 1, 600000).astype(np.float64)
    parts.append(dx * dx + dy * dy)
    dx, dy = rs.uniform(-BOX, BOX, 300000), rs.uniform(-BOX, BOX, 300000)
    parts.append(dx * dx + dy * dy)
    for lim in (3000.0, 2.0e6):                                   # the F32R range, integer and fractional
        dx, dy = rs.uniform(-lim, lim, 200000), rs.uniform(-lim, lim, 200000)
        parts.append(dx * dx + dy * dy)
        parts.append(np.rint(dx) ** 2 + np.rint(dy) ** 2)
    # where the rounding to an integer flips, and the perfect squares: at and one f32 step either side
    k = np.concatenate([rs.randint(1, 1 << 27, 150000), rs.randint(1, int(F32R_BOUND), 150000), np.arange(1, 2000)]).astype(np.float64)
    for mid in ((k + 0.5) * (k + 0.5), k * k):
        for off in (-1, 0, 1):
            parts.append(f32_step(mid, off).astype(np.float64))
    # the binade edges of the root: every power of two up to 2^53, two f32 neighbours on each side
    p = np.float32(2.0) ** np.arange(0, 54).astype(np.float32)
    for off in (-2, -1, 0, 1, 2):
        parts.append(f32_step(p, off).astype(np.float64))
    # the largest root the F32R form is used for, and its neighbours' squares
    top = f32_step(np.array([F32R_BOUND]), -1).astype(np.float64)
    parts.append(np.concatenate([top * top, f32_step(top * top, -1).astype(np.float64), f32_step(top * top, -2).astype(np.float64)]))
    sq = np.concatenate(parts)
    return sq[(sq >= 0) & (sq <= 2.0 ** 54)]


def test_corrected_root_gives_the_reference_weight_for_every_admissible_root():
    sq = samples()
    w = want(sq)
    assert len(sq) > 1000000 and sq.min() == 0.0 and w.max() > 134000000
    for ulps in (0, -1, 1):
        got = weight(sq, ulps, False)
        bad = np.nonzero(got != w)[0]
        assert len(bad) == 0, (ulps, sq[bad[:5]], got[bad[:5]], w[bad[:5]])


def test_f32_rounding_form_is_exact_below_its_guard():
    """F32R: c + 0.5f is representable while c < 2^22, so the f32 addition rounds nothing; only roots below 4.0e6 reach it"""
    sq = samples()
    sq = sq[np.sqrt(sq.astype(np.float32)) < np.float32(F32R_BOUND)]
    w = want(sq)
    top = float(f32_step(np.array([F32R_BOUND]), -1)[0])
    assert len(sq) > 1000000 and (sq == top * top).any() and w.max() == int(F32R_BOUND)
    for ulps in (0, -1, 1):
        got = weight(sq, ulps, True)
        bad = np.nonzero(got != w)[0]
        assert len(bad) == 0, (ulps, sq[bad[:5]], got[bad[:5]], w[bad[:5]])


def test_the_selects_restore_the_correctly_rounded_root():
    """what the two residuals are for: whichever of the three admissible roots the hardware returns, c is sqrtf(x)"""
    sq = samples()
    x = sq.astype(np.float32)
    exact = np.sqrt(x)
    for ulps in (0, -1, 1):
        r = f32_step(exact, ulps)
        ri = r.view(np.int32)
        rm, rp = (ri - 1).view(np.float32), (ri + 1).view(np.float32)
        X, R = x.astype(np.float64), r.astype(np.float64)
        with np.errstate(invalid="ignore"):
            c = np.where(0.0 >= X - rm.astype(np.float64) * R, rm, r)
            c = np.where(0.0 < X - rp.astype(np.float64) * R, rp, c).astype(np.float32)
        ok = (c == exact) | (x == 0)           # x = 0 moved off zero is no root the hardware returns (sqrt(0) = 0 exactly)
        assert ok.all(), (ulps, sq[~ok][:5])
