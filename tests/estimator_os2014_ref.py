"""Numpy restatement of the OS2014 localized estimator of BlockSWIPDG (the reference's Estimators::BlockSWIPDG,
dune/hdd/linearelliptic/estimators/block-swipdg.hh:118-328, 546-561, 721-890) on top of estimator_ref.estimate; the
yardstick of hdd_block_swipdg_estimate.

A segment is a contiguous element range [bounds[s], bounds[s + 1]); the segments partition [0, n).
Per element T:
  eta_NC,T^2, eta_DF,T^2   those of ESV2007 (estimator_ref.estimate), with theta_bar / theta_mu and theta_hat
  r_T = int_T (f - P0 f)^2  the two simplex rules of eta_R,T^2, without h_T^2 / (pi^2 lambda_min); with residual_star
                            div t_h stands for P0 f
  m_T = min(kappa_T(theta_min), kappa_T(theta_max)) lambda_min(A_T)
Per segment s:
  N_s = sum eta_NC,T^2, D_s = sum eta_DF,T^2, R_s = diam_s^2 / (pi^2 min m_T) sum r_T, diam_s the largest distance between
  two vertices of the segment's elements;
  indicator_s = 3 / sqrt(alpha_bar) (sqrt(gamma_bar) N_s + R_s + gamma_tilde D_s) / eta^2 (0 when eta = 0)
Global: eta_NC = sqrt(sum N_s), eta_R = sqrt(sum R_s), eta_DF = sqrt(sum D_s),
  eta = 1 / sqrt(alpha_bar) (sqrt(gamma_bar) eta_NC + eta_R + gamma_tilde eta_DF),
  alpha_bar = alpha(mu, mu_bar), gamma_bar = gamma(mu, mu_bar), gamma_tilde = max(sqrt(gamma(mu, mu_hat)),
  1 / sqrt(alpha(mu, mu_hat))), alpha(mu, mu') = min_q theta_q(mu) / theta_q(mu'), gamma = max_q of the same ratio.

In float64 the sums are the device's: a segment sum is estimator_ref.fixed_order_sum of the slice, the total over the
segments strided_total.  In np.longdouble they are plain sums: the gap between the two is what the device tests take
their tolerances from."""
import numpy as np

import estimator_ref as R


def strided_total(x, wg=256):
    """the device's sum over the segments: lane t adds the entries t, t + wg, ... in order, then the halving tree"""
    x = np.asarray(x, np.float64)
    acc = np.zeros(wg)
    for k in range(0, x.shape[0], wg):
        c = x[k:k + wg]
        acc[:c.shape[0]] += c
    s = wg // 2
    while s >= 1:
        acc[:s] += acc[s:2 * s]
        s //= 2
    return float(acc[0])


def segment_sums(x, bounds, dtype=np.float64):
    """the sum of every segment's slice of x: fixed_order_sum in float64, a plain sum in any other type"""
    if dtype is np.float64:
        return np.array([R.fixed_order_sum(x[a:b]) for a, b in zip(bounds[:-1], bounds[1:])])
    return np.array([x[a:b].sum() for a, b in zip(bounds[:-1], bounds[1:])], dtype)


def brute_force_diameters(coords, ev, bounds):
    """the reference's loop: the largest distance between two vertices of the segment's elements (float64)"""
    xy = np.asarray(coords, np.float64)
    ev = np.asarray(ev, np.int64)
    out = np.zeros(len(bounds) - 1)
    for s, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        p = xy[np.unique(ev[a:b].reshape(-1))]
        best = 0.0
        for k in range(0, p.shape[0], 512):
            d = p[k:k + 512, None, :] - p[None, :, :]
            best = max(best, float(np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).max()))
        out[s] = best
    return out


def factors(theta_mu, theta_bar=None, theta_hat=None, dtype=np.float64):
    """(alpha_bar, gamma_bar, alpha_hat, gamma_hat, gamma_tilde)"""
    T = dtype
    mu = np.asarray(theta_mu).astype(T)
    bar = mu if theta_bar is None else np.asarray(theta_bar).astype(T)
    hat = mu if theta_hat is None else np.asarray(theta_hat).astype(T)
    ab, gb = (mu / bar).min(), (mu / bar).max()
    ah, gh = (mu / hat).min(), (mu / hat).max()
    return ab, gb, ah, gh, max(np.sqrt(gh), T(1) / np.sqrt(ah))


def box_partition(coords, ev, px, py, lower=(-1.0, -1.0), upper=(1.0, 1.0)):
    """(perm, bounds): the elements sorted (stably) into px x py boxes of [lower, upper] by their centroids, x fastest --
    the subdomain-major numbering of a px x py partitioning -- and the element bounds of the boxes"""
    c = np.asarray(coords, np.float64)[np.asarray(ev, np.int64)].mean(1)
    ix = np.clip(((c[:, 0] - lower[0]) / (upper[0] - lower[0]) * px).astype(np.int64), 0, px - 1)
    iy = np.clip(((c[:, 1] - lower[1]) / (upper[1] - lower[1]) * py).astype(np.int64), 0, py - 1)
    box = iy * px + ix
    perm = np.argsort(box, kind="stable")
    counts = np.bincount(box, minlength=px * py)
    return perm, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def estimate_blocks(coords, ev, u, bounds, kappa=None, theta_mu=None, theta_bar=None, theta_hat=None, theta_min=None,
                    theta_max=None, tensor=None, force=None, sigma_inner=8.0, sigma_boundary=14.0, beta=1.0,
                    residual_star=False, diam=None, dtype=np.float64):
    """arguments as estimator_ref.estimate, and: bounds [S + 1]; theta_min / theta_max (None: theta_mu); diam [S] (None:
    brute force).  Returns a dict: local [4, ne] (eta_NC^2, r_T, eta_DF^2, m_T), segments [4, S] (N_s, R_s, D_s,
    indicator), sums [4] (sum N_s, sum R_s, sum D_s, eta^2), eta_nc, eta_r, eta_df, eta, factors, diam, flux, oswald."""
    T = dtype
    esv = R.estimate(coords, ev, u, kappa=kappa, theta_mu=theta_mu, theta_bar=theta_bar, theta_hat=theta_hat, tensor=tensor,
                     force=force, sigma_inner=sigma_inner, sigma_boundary=sigma_boundary, beta=beta,
                     residual_star=residual_star, dtype=T)
    xy = np.asarray(coords).astype(T)
    ev = np.asarray(ev, np.int64)
    ne = ev.shape[0]
    bounds = np.asarray(bounds, np.int64)
    assert bounds[0] == 0 and bounds[-1] == ne and np.all(np.diff(bounds) > 0)
    kap = np.ones((1, ne), T) if kappa is None else np.asarray(kappa).astype(T).reshape(-1, ne)
    nq = kap.shape[0]
    th_mu = np.ones(nq, T) if theta_mu is None else np.asarray(theta_mu).astype(T)
    th_min = th_mu if theta_min is None else np.asarray(theta_min).astype(T)
    th_max = th_mu if theta_max is None else np.asarray(theta_max).astype(T)
    if tensor is None:
        A = np.stack([np.ones(ne, T), np.zeros(ne, T), np.ones(ne, T)])
    else:
        A = np.asarray(tensor).astype(T)
        if A.ndim == 1:
            A = np.repeat(A[:, None], ne, 1)
    # r_T
    p = xy[ev]
    det = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 2, 0] - p[:, 0, 0]) * (p[:, 1, 1] - p[:, 0, 1])

    def force_at(rule):
        P, w = R.simplex_rule(rule, T)
        x = p[:, 0, 0, None] + (p[:, 1, 0] - p[:, 0, 0])[:, None] * P[None, :, 0] + (p[:, 2, 0] - p[:, 0, 0])[:, None] * P[None, :, 1]
        y = p[:, 0, 1, None] + (p[:, 1, 1] - p[:, 0, 1])[:, None] * P[None, :, 0] + (p[:, 2, 1] - p[:, 0, 1])[:, None] * P[None, :, 1]
        return (np.zeros_like(x) if force is None else force(x, y)), w

    order = 0 if force is None else force.order
    if force is None and not residual_star:
        r = np.zeros(ne, T)
    else:
        if residual_star:
            mean = esv["div"]
        else:
            fa, wa = force_at(order + 2)
            mean = T(2) * (fa * wa[None, :]).sum(1)
        fb, wb = force_at(2 * order + 2)
        r = np.abs(det) * (((fb - mean[:, None]) ** 2) * wb[None, :]).sum(1)
    # m_T
    lam = (A[0] + A[2]) / T(2) - np.sqrt(((A[0] - A[2]) / T(2)) ** 2 + A[1] ** 2)
    m = np.minimum((th_min[:, None] * kap).sum(0), (th_max[:, None] * kap).sum(0)) * lam
    local = np.stack([esv["local"][0], r, esv["local"][2], m])
    # segments
    if diam is None:
        diam = brute_force_diameters(coords, ev, bounds)
    d = np.asarray(diam).astype(T)
    N = segment_sums(local[0], bounds, T)
    D = segment_sums(local[2], bounds, T)
    mins = np.array([m[a:b].min() for a, b in zip(bounds[:-1], bounds[1:])], T)
    Rs = d * d / (R._pi(T) ** 2 * mins) * segment_sums(r, bounds, T)
    ab, gb, ah, gh, gt = factors(th_mu, theta_bar, theta_hat, T)
    total = (lambda x: T(strided_total(x))) if T is np.float64 else (lambda x: x.sum())
    sN, sR, sD = total(N), total(Rs), total(D)
    eta = (T(1) / np.sqrt(ab)) * (np.sqrt(gb) * np.sqrt(sN) + np.sqrt(sR) + gt * np.sqrt(sD))
    ind = T(3) / np.sqrt(ab) * (np.sqrt(gb) * N + Rs + gt * D)
    ind = ind / (eta * eta) if eta > 0 else np.zeros_like(ind)      # eta = 0: every indicator is 0
    return dict(local=local, segments=np.stack([N, Rs, D, ind]), sums=np.array([sN, sR, sD, eta * eta], T),
                eta_nc=np.sqrt(sN), eta_r=np.sqrt(sR), eta_df=np.sqrt(sD), eta=eta, factors=(ab, gb, ah, gh, gt), diam=d,
                flux=esv["flux"], oswald=esv["oswald"], esv=esv)
