"""Shared by the calibration tests (msv.h "Calibration"): float64 restatements of the fits with
math.fsum, the bounds DESIGN 4.15 derives, the seeded Gumbel sample and the bit score's float32 expression.

Bounds (u = 2^-53, all from the arithmetic, none from what the code gives):

  location   |d mu| <= (n + 8) u / lambda + 4 u |mu|.  S0 is a sum of n positive terms: any order of n - 1 float64
             adds has relative error below n u, each exp adds under 2 u (1 ulp in either library), the division by n
             one more; log turns the relative error of its argument into an absolute one of the same size plus u |log|,
             the division by lambda scales it, and the subtraction from x_min and the division round |mu|-sized values.
  complete   the two sides stop within their own Newton step of their own root.  The step that ends the loop is at most
             1e-9 lambda, and Newton's error after a step s is |f'' / (2 f')| s^2.  With V and m3 the variance and the
             third central moment of y under the weights exp(-l y), f' = -(V + 1 / l^2) and f'' = 2 / l^3 + m3 with
             |m3| <= y_max V, so |f'' / f'| <= 2 / lambda + y_max and the left-over is below
             (1 / lambda + y_max / 2) 1e-18 lambda^2.  The roots differ by the rounding of f over |f'|:
             f = 1 / l - ybar + S1 / S0 carries (3 n + 8) u max(ybar, 1 / lambda) (three sums of n positive terms,
             S1 / S0 <= ybar at the root), so
                 |d lambda| <= 2 ((1 / lambda + y_max / 2) 1e-18 lambda^2 + (3 n + 8) u max(ybar, 1 / lambda) / |f'|)
             -- the issue's n 2^-50 / |f'| with the scale of f written out -- and mu follows through
             d mu / d lambda = (x_min - mu) / lambda ... (|x_min - mu| + ybar) / lambda bounds it:
                 |d mu| <= location bound + (|x_min - mu| + ybar) / lambda |d lambda|
  tau        tau = gmu - log(-log(1 - t)) / glam + log(t) / lambda_p:
                 |d tau| <= |d gmu| + |log(-log(1 - t))| / glam^2 |d glam| + 8 u (|tau| + |log t| / lambda_p)
"""
import math

import numpy as np

U = 2.0 ** -53
LN2F = np.float32(0.69314718055994529)


def gumbel_sample(seed: int, n: int, mu: float, lam: float) -> np.ndarray:
    """n float32 draws of Gumbel(mu, lambda), PCG64(seed)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (mu + rng.gumbel(size=n) / lam).astype(np.float32)


def null1_score(L: int) -> np.float32:
    p1 = np.float32(L) / np.float32(L + 1)
    return np.float32(L * math.log(float(p1)) + math.log(1.0 - float(p1)))


def bit_scores(scores, L: int) -> np.ndarray:
    """The float32 bit scores the fits run on: fwd_host.h's bits_of(score - null1_score(L)); L = 0: as they are."""
    s = np.asarray(scores, np.float32)
    return s if L == 0 else (s - null1_score(L)) / LN2F


def ref_location(x32, lam: float) -> float:
    x = np.asarray(x32, np.float64)
    xmin = float(x.min())
    s0 = math.fsum(math.exp(-lam * float(v - xmin)) for v in x)
    return xmin - math.log(s0 / len(x)) / lam


def location_bound(n: int, lam: float, mu: float) -> float:
    return (n + 8) * U / lam + 4 * U * abs(mu)


def lawless(x32, lam: float):
    """(f, f', ybar, x_min, y_max) of the complete fit's equation at lambda, float64 with fsum."""
    x = np.asarray(x32, np.float64)
    xmin = float(x.min())
    y = [float(v - xmin) for v in x]
    ybar = math.fsum(y) / len(y)
    e = [math.exp(-lam * v) for v in y]
    s0 = math.fsum(e)
    s1 = math.fsum(v * w for v, w in zip(y, e))
    s2 = math.fsum(v * v * w for v, w in zip(y, e))
    r = s1 / s0
    return 1.0 / lam - ybar + r, r * r - s2 / s0 - 1.0 / (lam * lam), ybar, xmin, max(y)


def gumbel_bounds(x32, mu: float, lam: float):
    """(|d mu|, |d lambda|) allowed between two runs of the complete fit on the same float32 scores."""
    n = len(x32)
    _, df, ybar, xmin, ymax = lawless(x32, lam)
    dlam = 2.0 * ((1.0 / lam + ymax / 2) * 1e-18 * lam * lam + (3 * n + 8) * U * max(ybar, 1.0 / lam) / abs(df))
    dmu = location_bound(n, lam, mu) + (abs(xmin - mu) + ybar) / lam * dlam
    return dmu, dlam


def ref_tau(gmu: float, glam: float, lam: float, tail: float) -> float:
    return gmu - math.log(-math.log(1.0 - tail)) / glam + math.log(tail) / lam


def tau_bound(dmu: float, dlam: float, glam: float, lam: float, tail: float, tau: float) -> float:
    return dmu + abs(math.log(-math.log(1.0 - tail))) / (glam * glam) * dlam + \
        8 * U * (abs(tau) + abs(math.log(tail)) / lam)
