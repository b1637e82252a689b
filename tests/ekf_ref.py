"""EKF.estimate of the package's ekf_lm.py restated operation by operation in mpmath at 50 digits (test infrastructure
only; imported by tests/test_filter_cases.py and by hand, never by a gpu test).

Every input enters as the float64 it is (mpf(float)), the constants of ekf_lm.py included - Cx as NumPy squares it,
math.pi, M_DIST_TH - so the answer is the true result of the reference's formulas on the same numbers.  Kept as the
reference has them: the dense H, the literal (I - K H) P, pi_2_pi as Python's %, the n1 that is never refreshed, the early
return before the yaw wrap, and the hstack that raises.  The products skip the entries of H and of I - K H that are
exact zeros, and leave out the columns of H P that nothing reads: an exact zero times a finite number adds an exact zero
at any precision, so the sums are those of the dense products.  The inverse of the 2 x 2 S is its adjugate over its determinant.

    run(u, z, x0=None, max_lm=None) -> [step]    one entry per step that was started, each a dict:
        x, P        lists of mpf after the step (before it, when the step raised)
        nlm         landmarks in the state
        status      0, 1 when the reference raises ValueError in this step, or 2 when `max_lm` is given and the step would
                    append a landmark past it (slam_ekf_lm's stop); a step of status 1 or 2 is the last entry
        rows        per observation row that was looked at: (dists with the threshold entry last, chosen index, branch),
                    branch one of "matched", "appended", "early", "raises"
"""
import math

import numpy as np
from mpmath import mp, mpf

DIGITS = 50
mp.dps = DIGITS

PI = mpf(math.pi)
TH = mpf(0.6)                                                   # M_DIST_TH
CX = [mpf(float(v)) for v in np.diag(np.diag([0.35, 0.35, np.deg2rad(15.0)]) ** 2)]
ZERO, ONE = mpf(0), mpf(1)


def pi_2_pi(a):
    """(a + math.pi) % (2 * math.pi) - math.pi with Python's %, whose result takes the sign of the divisor."""
    b = 2 * PI
    v = a + PI
    return v - mp.floor(v / b) * b - PI


def correction(x, P, zr, zb, i):
    """laser_correction for landmark i: (y, S, H) with H dense, 2 x len(x)."""
    n = len(x)
    dx, dy = x[3 + 2 * i] - x[0], x[4 + 2 * i] - x[1]
    q = dx * dx + dy * dy
    za = mp.atan2(dy, dx) - x[2]
    sq = mp.sqrt(q)
    y = [zr - sq, pi_2_pi(zb - pi_2_pi(za))]
    g = [[-sq * dx / q, -sq * dy / q, ZERO / q, sq * dx / q, sq * dy / q], [dy / q, -dx / q, -q / q, -dy / q, dx / q]]
    H = [[ZERO] * n, [ZERO] * n]
    for r in range(2):
        H[r][0], H[r][1], H[r][2] = g[r][:3]
        H[r][3 + 2 * i], H[r][4 + 2 * i] = g[r][3:]
    cols = [c for c in range(n) if H[0][c] != 0 or H[1][c] != 0]
    HP = [{c: sum((H[r][k] * P[k][c] for k in cols), ZERO) for c in cols} for r in range(2)]     # the columns S reads
    S = [[sum((HP[r][k] * H[r2][k] for k in cols), ZERO) + (CX[r] if r == r2 else ZERO) for r2 in range(2)] for r in range(2)]
    return y, S, H, cols


def inverse(S):
    det = S[0][0] * S[1][1] - S[0][1] * S[1][0]
    return [[S[1][1] / det, -S[0][1] / det], [-S[1][0] / det, S[0][0] / det]]


def distances(x, P, zr, zb):
    """min_dist of search_correspond_landmark_id: one Mahalanobis distance per landmark, then the threshold."""
    out = []
    for i in range((len(x) - 3) // 2):
        y, S, _, _ = correction(x, P, zr, zb, i)
        Si = inverse(S)
        t0, t1 = y[0] * Si[0][0] + y[1] * Si[1][0], y[0] * Si[0][1] + y[1] * Si[1][1]
        out.append(t0 * y[0] + t1 * y[1])
    out.append(TH)
    return out


class Raises(Exception):
    pass


class Capped(Exception):
    pass


def estimate(x, P, rows, u, log, max_lm=None):
    """EKF.estimate on lists of mpf; returns the new (x, P).  Raises ``Raises`` where np.hstack would, and ``Capped`` where
    the state would grow past ``max_lm`` landmarks (slam_ekf_lm's own stop; None: the reference alone)."""
    n1 = len(x)
    yaw, ux, uy, uw = x[2], u[0], u[1], u[2]
    c, s = mp.cos(yaw), mp.sin(yaw)
    G = [[ONE, ZERO, -s * ux - c * uy], [ZERO, ONE, c * ux - s * uy], [ZERO, ZERO, ONE]]
    x = [x[0] + c * ux - s * uy, x[1] + s * ux + c * uy, yaw + uw] + list(x[3:])
    A = [[sum((G[k][i] * P[k][j] for k in range(3)), ZERO) for j in range(3)] for i in range(3)]
    R = [[sum((A[i][k] * G[k][j] for k in range(3)), ZERO) + (CX[i] if i == j else ZERO) for j in range(3)] for i in range(3)]
    P = [list(row) for row in P]
    for i in range(3):
        P[i][:3] = R[i]
    for zr, zb in rows:
        num_lm = (n1 - 3) // 2
        dists = distances(x, P, zr, zb)
        best = dists.index(min(dists))
        if num_lm == best:
            if len(P) != n1:                                        # hstack of n1 + 2 and n1 rows
                log.append((dists, best, "raises"))
                raise Raises()
            if max_lm is not None and num_lm == max_lm:
                log.append((dists, best, "appended"))
                raise Capped()
            a = x[2] + zb
            x = x + [x[0] + zr * mp.cos(a), x[1] + zr * mp.sin(a)]
            P = [row + [ZERO, ZERO] for row in P] + [[ZERO] * n1 + [ONE, ZERO], [ZERO] * n1 + [ZERO, ONE]]
            branch = "appended"
        elif 3 + 2 * best >= len(x):                                # get_landmark_position_from_state is empty
            log.append((dists, best, "early"))
            return x, P
        else:
            branch = "matched"
        log.append((dists, best, branch))
        n = len(x)
        y, S, H, cols = correction(x, P, zr, zb, best)
        Si = inverse(S)
        PHt = [[sum((P[r][k] * H[j][k] for k in cols), ZERO) for j in range(2)] for r in range(n)]
        K = [[PHt[r][0] * Si[0][j] + PHt[r][1] * Si[1][j] for j in range(2)] for r in range(n)]
        x = [x[r] + (K[r][0] * y[0] + K[r][1] * y[1]) for r in range(n)]
        M = {}                                                      # I - K H, its entries that are not exact zeros
        for r in range(n):
            for k in set(cols) | {r}:
                M[r, k] = (ONE if r == k else ZERO) - (K[r][0] * H[0][k] + K[r][1] * H[1][k])
        live = [sorted(set(cols) | {r}) for r in range(n)]
        P = [[sum((M[r, k] * P[k][cc] for k in live[r]), ZERO) for cc in range(n)] for r in range(n)]
    x[2] = pi_2_pi(x[2])
    return x, P


def run(u, z, x0=None, max_lm=None):
    x = [mpf(float(v)) for v in (x0 if x0 is not None else (0.0, 0.0, 0.0))]
    P = [[ONE if i == j else ZERO for j in range(3)] for i in range(3)]
    out = []
    for us, zs in zip(u, z):
        rows = [(mpf(float(r[0])), mpf(float(r[1]))) for r in np.asarray(zs, dtype=np.float64).reshape(-1, 2)]
        log = []
        try:
            x, P = estimate(x, P, rows, [mpf(float(v)) for v in us], log, max_lm)
        except (Raises, Capped) as e:
            out.append(dict(x=x, P=P, nlm=(len(x) - 3) // 2, status=1 if isinstance(e, Raises) else 2, rows=log))
            break
        out.append(dict(x=x, P=P, nlm=(len(x) - 3) // 2, status=0, rows=log))
    return out


def margin(rows):
    """The smallest gap between the winning entry and the runner-up over the decisions of ``rows`` (inf: none had two)."""
    best = mpf("inf")
    for dists, _, _ in rows:
        if len(dists) > 1:
            a = sorted(dists)
            best = min(best, a[1] - a[0])
    return best
