"""Numpy restatement of the ESV2007 a-posteriori estimator for P1 SWIPDG on conforming triangles, as the reference's
Estimators::SWIPDG computes it (dune/hdd/linearelliptic/estimators/swipdg.hh); the yardstick of the device estimator.

Definitions (u_h the P1 DG vector, DoF 3e + i at vertex ev[e, i]; K_T(theta) = kappa_T(theta) A_T, constant on T;
faces of T: f0 = (v0, v1), f1 = (v0, v2), f2 = (v1, v2), face f opposite vertex 2 - f; every boundary face Dirichlet,
g_D = 0):
  Oswald     I_OS u_h: at a vertex the arithmetic mean of the DG values of the elements around it, 0 on the boundary
  eta_NC,T^2 = |T| g^T K_T(theta_bar) g,  g = grad(u_h - I_OS u_h)
  eta_R,T^2  = h_T^2 / (pi^2 lambda_min(K_T(theta_mu))) int_T (f - P0 f)^2,  h_T the longest edge, P0 f the element mean
               by the simplex rule of order ord(f) + 2, the integral by the rule of order 2 ord(f) + 2
  F_T,e      = -|e| (w- K- grad u- + w+ K+ grad u+) . n + (sigma_in gamma / |e|^beta) int_e (u- - u+)   (interior)
               -|e| K grad u . n + (sigma_bnd delta / |e|^beta) int_e u                                  (boundary)
               delta+- = n . K+-(theta_mu) n, w- = delta+ / (delta+ + delta-), w+ = delta- / (delta+ + delta-),
               gamma = delta+ delta- / (delta+ + delta-)
  t_h(x)     = sum_e F_T,e / (2 |T|) (x - p_e), p_e the vertex opposite e   (RT0)
  eta_DF,T^2 = int_T (grad u_h + Khat^-1 t_h)^T Khat (grad u_h + Khat^-1 t_h), Khat = K_T(theta_hat), by the three edge
               midpoints (exact)
  eta_T^2    = eta_NC,T^2 + (eta_R,T + eta_DF,T)^2
The simplex rules are the library's (csrc/host/quadrature.cpp simplex_rule), restated for any float type.

Everything is vectorised over the elements and runs in the float type `dtype` (np.float64 or np.longdouble): the
gap between the two is what the device tests take their tolerances from."""
import numpy as np

FV = ((0, 1), (0, 2), (1, 2))     # local vertices of face f
OPP = (2, 1, 0)                   # vertex opposite face f


def _pi(T):
    return T(np.pi) if T is np.float64 else T(4) * np.arctan(T(1))


def gauss_legendre01(n, dtype=np.float64):
    """n-point Gauss-Legendre rule on [0, 1], points ascending (Newton on P_n)"""
    T = dtype
    pi = _pi(T)
    x = np.cos(pi * (np.arange(n, 0, -1, dtype=T) - T(0.25)) / (T(n) + T(0.5)))
    for _ in range(100):
        p0, p1 = np.ones(n, T), x.copy()
        for k in range(2, n + 1):
            p0, p1 = p1, ((T(2 * k - 1)) * x * p1 - T(k - 1) * p0) / T(k)
        dp = T(n) * (x * p1 - p0) / (x * x - T(1))
        dx = p1 / dp
        x = x - dx
        if np.max(np.abs(dx)) < T(4) * np.finfo(T).eps:
            break
    p0, p1 = np.ones(n, T), x.copy()
    for k in range(2, n + 1):
        p0, p1 = p1, ((T(2 * k - 1)) * x * p1 - T(k - 1) * p0) / T(k)
    dp = T(n) * (x * p1 - p0) / (x * x - T(1))
    w = T(2) / ((T(1) - x * x) * dp * dp)
    return (x + T(1)) / T(2), w / T(2)


def simplex_rule(order, dtype=np.float64):
    """points [nq, 2] and weights [nq] (sum 1/2) on the reference triangle, exact for `order`"""
    T = dtype
    if order <= 1:
        return np.array([[T(1) / T(3), T(1) / T(3)]], T), np.array([T(0.5)], T)
    if order == 2:
        a, b = T(1) / T(6), T(2) / T(3)
        return np.array([[a, a], [b, a], [a, b]], T), np.full(3, T(1) / T(6), T)
    if order <= 4:
        a, wa = T("0.44594849091596488632"), T("0.22338158967801146570")
        b, wb = T("0.091576213509770743460"), T("0.10995174365532186764")
        one = T(1)
        P = np.array([[a, a], [one - 2 * a, a], [a, one - 2 * a], [b, b], [one - 2 * b, b], [b, one - 2 * b]], T)
        return P, T(0.5) * np.array([wa, wa, wa, wb, wb, wb], T)
    n = (order + 3) // 2
    s, w = gauss_legendre01(n, T)
    si, sj = np.repeat(s, n), np.tile(s, n)
    wi, wj = np.repeat(w, n), np.tile(w, n)
    return np.stack([si, sj * (T(1) - si)], 1), wi * wj * (T(1) - si)


def face_neighbors(ev):
    """neighbors [ne, 3] (-1: boundary face) of a conforming triangulation, by the sorted vertex ids of each face"""
    ev = np.asarray(ev, np.int64)
    ne = ev.shape[0]
    nv = int(ev.max()) + 1
    key = np.empty((ne, 3), np.int64)
    for f in range(3):
        a, b = ev[:, FV[f][0]], ev[:, FV[f][1]]
        key[:, f] = np.minimum(a, b) * nv + np.maximum(a, b)
    flat = key.reshape(-1)
    order = np.argsort(flat, kind="stable")
    sk = flat[order]
    nbr = np.full(3 * ne, -1, np.int64)
    same = np.nonzero(sk[1:] == sk[:-1])[0]
    nbr[order[same]] = order[same + 1] // 3
    nbr[order[same + 1]] = order[same] // 3
    return nbr.reshape(ne, 3)


def esv2007_force(dtype=np.float64):
    """ESV2007 Testcase1Force, 1/2 pi^2 cos(pi x / 2) cos(pi y / 2), integration order 3"""
    T = dtype
    pi = _pi(T)

    def f(x, y):
        return (pi * pi / T(2)) * np.cos(pi / T(2) * x) * np.cos(pi / T(2) * y)
    f.order = 3
    return f


def estimate(coords, ev, u, kappa=None, theta_mu=None, theta_bar=None, theta_hat=None, tensor=None, force=None,
             sigma_inner=8.0, sigma_boundary=14.0, beta=1.0, residual_star=False, dtype=np.float64):
    """coords [nv, 2], ev [ne, 3], u [3 ne]; kappa [n_comp, ne] (None: 1); tensor None (identity), (a11, a12, a22) or
    [3, ne]; force: None or a callable f(x, y) with an attribute `order`; residual_star: eta_R_ESV2007_* in place of
    eta_R (div t_h = sum_e F_T,e / |T| stands for P0 f, a missing force is f = 0).  Returns a dict: local [4, ne] (eta_NC^2,
    eta_R^2, eta_DF^2, eta_T^2), flux [3, ne], oswald [nv], div [ne] (sum_e F_T,e / |T|), sums [4], eta, eta_alt."""
    T = dtype
    xy = np.asarray(coords).astype(T)
    ev = np.asarray(ev, np.int64)
    ne, nv = ev.shape[0], xy.shape[0]
    uu = np.asarray(u).astype(T).reshape(ne, 3)
    kap = np.ones((1, ne), T) if kappa is None else np.asarray(kappa).astype(T).reshape(-1, ne)
    nq = kap.shape[0]
    th_mu = np.ones(nq, T) if theta_mu is None else np.asarray(theta_mu).astype(T)
    th_bar = th_mu if theta_bar is None else np.asarray(theta_bar).astype(T)
    th_hat = th_mu if theta_hat is None else np.asarray(theta_hat).astype(T)
    if tensor is None:
        A = np.stack([np.ones(ne, T), np.zeros(ne, T), np.ones(ne, T)])
    else:
        A = np.asarray(tensor).astype(T)
        if A.ndim == 1:
            A = np.repeat(A[:, None], ne, 1)

    def Kof(theta):
        k = (theta[:, None] * kap).sum(0)
        return k * A[0], k * A[1], k * A[2]

    nbr = face_neighbors(ev)
    # Oswald interpolation
    cnt = np.bincount(ev.reshape(-1), minlength=nv).astype(T)
    tot = np.zeros(nv, T)
    np.add.at(tot, ev.reshape(-1), uu.reshape(-1))
    osw = tot / np.maximum(cnt, T(1))
    bnd = np.zeros(nv, bool)
    for f in range(3):
        on = nbr[:, f] < 0
        bnd[ev[on, FV[f][0]]] = True
        bnd[ev[on, FV[f][1]]] = True
    osw[bnd] = T(0)

    p = xy[ev]                                   # [ne, 3, 2]
    det = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 2, 0] - p[:, 0, 0]) * (p[:, 1, 1] - p[:, 0, 1])
    area = np.abs(det) / T(2)
    # gradients of the barycentric coordinates [ne, 3, 2]
    gl = np.stack([np.stack([p[:, 1, 1] - p[:, 2, 1], p[:, 2, 0] - p[:, 1, 0]], 1),
                   np.stack([p[:, 2, 1] - p[:, 0, 1], p[:, 0, 0] - p[:, 2, 0]], 1),
                   np.stack([p[:, 0, 1] - p[:, 1, 1], p[:, 1, 0] - p[:, 0, 0]], 1)], 1) / det[:, None, None]

    def grad(v):                                 # v [ne, 3] -> [ne, 2]
        return (v[:, :, None] * gl).sum(1)

    def quad(K, a, b):                           # a^T K b
        return K[0] * a[:, 0] * b[:, 0] + K[1] * (a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]) + K[2] * a[:, 1] * b[:, 1]

    def mul(K, a):
        return np.stack([K[0] * a[:, 0] + K[1] * a[:, 1], K[1] * a[:, 0] + K[2] * a[:, 1]], 1)

    Kmu, Kbar, Khat = Kof(th_mu), Kof(th_bar), Kof(th_hat)
    g = grad(uu)
    # nonconformity
    gd = grad(uu - osw[ev])
    eta_nc2 = area * quad(Kbar, gd, gd)
    # residual
    el = [np.hypot(p[:, b, 0] - p[:, a, 0], p[:, b, 1] - p[:, a, 1]) for a, b in FV]
    h = np.maximum(np.maximum(el[0], el[1]), el[2])
    lam = (Kmu[0] + Kmu[2]) / T(2) - np.sqrt(((Kmu[0] - Kmu[2]) / T(2)) ** 2 + Kmu[1] ** 2)
    def force_at(rule):
        P, w = simplex_rule(rule, T)
        x = p[:, 0, 0, None] + (p[:, 1, 0] - p[:, 0, 0])[:, None] * P[None, :, 0] + (p[:, 2, 0] - p[:, 0, 0])[:, None] * P[None, :, 1]
        y = p[:, 0, 1, None] + (p[:, 1, 1] - p[:, 0, 1])[:, None] * P[None, :, 0] + (p[:, 2, 1] - p[:, 0, 1])[:, None] * P[None, :, 1]
        return (np.zeros_like(x) if force is None else force(x, y)), w

    def residual2(div):
        order = 0 if force is None else force.order
        if residual_star:
            mean = div
        elif force is None:
            return np.zeros(ne, T)
        else:
            fa, wa = force_at(order + 2)
            mean = T(2) * (fa * wa[None, :]).sum(1)
        fb, wb = force_at(2 * order + 2)
        return h * h / (_pi(T) ** 2 * lam) * np.abs(det) * (((fb - mean[:, None]) ** 2) * wb[None, :]).sum(1)
    # diffusive flux reconstruction
    F = np.zeros((3, ne), T)
    for f in range(3):
        a, b = FV[f]
        o = OPP[f]
        t = p[:, b] - p[:, a]
        le = np.hypot(t[:, 0], t[:, 1])
        n = np.stack([t[:, 1], -t[:, 0]], 1) / le[:, None]
        sgn = np.where(((p[:, a] - p[:, o]) * n).sum(1) > 0, T(1), T(-1))
        n = n * sgn[:, None]
        N = nbr[:, f]
        inner = N >= 0
        Nn = np.where(inner, N, 0)
        dm = quad(Kmu, n, n)
        Kp = (Kmu[0][Nn], Kmu[1][Nn], Kmu[2][Nn])
        dp = quad(Kp, n, n)
        wm, wp, gam = dp / (dp + dm), dm / (dp + dm), dp * dm / (dp + dm)
        mean_m = (uu[:, a] + uu[:, b]) / T(2)
        # the neighbour's trace on the edge: its DoFs at the two shared vertices
        shared = (ev[Nn][:, :, None] == np.stack([ev[:, a], ev[:, b]], 1)[:, None, :]).any(2)    # [ne, 3]
        mean_p = (uu[Nn] * shared).sum(1) / T(2)
        flux_in = -le * ((wm[:, None] * mul(Kmu, g) + wp[:, None] * mul(Kp, g[Nn])) * n).sum(1) \
            + T(sigma_inner) * gam / le ** T(beta) * le * (mean_m - mean_p)
        flux_bd = -le * (mul(Kmu, g) * n).sum(1) + T(sigma_boundary) * dm / le ** T(beta) * le * mean_m
        F[f] = np.where(inner, flux_in, flux_bd)
    # diffusive flux estimator at the three edge midpoints
    dK = Khat[0] * Khat[2] - Khat[1] * Khat[1]
    Kinv = (Khat[2] / dK, -Khat[1] / dK, Khat[0] / dK)
    eta_df2 = np.zeros(ne, T)
    for a, b in FV:
        m = (p[:, a] + p[:, b]) / T(2)
        th = np.zeros((ne, 2), T)
        for f in range(3):
            th = th + (F[f] / (T(2) * area))[:, None] * (m - p[:, OPP[f]])
        w = g + mul(Kinv, th)
        eta_df2 = eta_df2 + area / T(3) * quad(Khat, w, w)
    eta_r2 = residual2(F.sum(0) / area)
    eta_t2 = eta_nc2 + (np.sqrt(eta_r2) + np.sqrt(eta_df2)) ** 2
    local = np.stack([eta_nc2, eta_r2, eta_df2, eta_t2])
    sums = local.sum(1)
    return dict(local=local, flux=F, oswald=osw, div=F.sum(0) / area, area=area, sums=sums,
                eta=np.sqrt(sums[3]), eta_alt=np.sqrt(sums[0]) + np.sqrt(sums[1]) + np.sqrt(sums[2]), neighbors=nbr)


def fixed_order_sum(x, wg=256):
    """the device's two-stage sum of a float64 array: per workgroup of `wg` consecutive elements a halving tree
    (v[t] += v[t + s], s = wg/2 .. 1; missing elements are 0), then one workgroup in which lane t adds the partial
    sums t, t + wg, ... in order, and the same tree"""
    def tree(a):
        a = a.copy()
        s = wg // 2
        while s >= 1:
            a[:, :s] += a[:, s:2 * s]
            s //= 2
        return a[:, 0]
    x = np.asarray(x, np.float64)
    nwg = max(1, -(-x.shape[0] // wg))
    pad = np.zeros(nwg * wg)
    pad[:x.shape[0]] = x
    part = tree(pad.reshape(nwg, wg))
    acc = np.zeros(wg)
    for k in range(0, nwg, wg):
        c = part[k:k + wg]
        acc[:c.shape[0]] += c
    return float(tree(acc.reshape(1, wg))[0])
