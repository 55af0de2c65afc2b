"""Float64 numpy statement of the sampling path without the occupancy grid (csrc/hiersample.hip; DESIGN.md "The sampling path
without the grid"): stratified samples, inverse-CDF upsampling with the depth merge, weights, compositing and the compositing's
backward.  Written from the formulae of include/seal3d_hip.h, not from the kernels.  S = num_steps, U = upsample_steps, K = S + U;
sigma, rgbs, weights, mask and the gradients are in the concatenated [coarse | fine] order, `order` maps sorted slots to columns."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


def f64(x):
    return np.asarray(x, dtype=np.float64)


def near_far(rays_o, rays_d, aabb, min_near):
    """slab test against the box, near clamped to min_near; a miss gives FLT_MAX twice"""
    o, d, a = f64(rays_o), f64(rays_d), f64(aabb)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (a[:3] - o) / d, (a[3:] - o) / d
    lo, hi = np.minimum(t0, t1), np.maximum(t0, t1)
    near, far = lo.max(axis=1), hi.min(axis=1)
    miss = near > far
    near = np.maximum(near, min_near)
    return np.where(miss, FLT_MAX, near), np.where(miss, FLT_MAX, far)


def points(rays_o, rays_d, z, aabb):
    a = f64(aabb)
    return np.clip(f64(rays_o)[:, None, :] + f64(rays_d)[:, None, :] * f64(z)[:, :, None], a[:3], a[3:])


def coarse_samples(rays_o, rays_d, aabb, min_near, S, noise=None):
    """nears, fars [N], z [N, S], xyz [N, S, 3]"""
    near, far = near_far(rays_o, rays_d, aabb, min_near)
    z = near[:, None] + (far - near)[:, None] * np.linspace(0.0, 1.0, S)[None, :]
    if noise is not None:
        z = z + (f64(noise) - 0.5) * ((far - near) / S)[:, None]
    return near, far, z, points(rays_o, rays_d, z, aabb)


def alpha_weights(z, sigma, nears, fars, scale, S):
    """delta (the last one (far - near) / S), alpha, s = 1 - alpha + 1e-15, T = exclusive product of s, w = alpha T, exp(-x)"""
    z, sigma = f64(z), f64(sigma)
    last = ((f64(fars) - f64(nears)) / S)[:, None]
    delta = np.concatenate([z[:, 1:] - z[:, :-1], last], axis=1)
    e = np.exp(-delta * scale * sigma)
    alpha = 1.0 - e
    s = 1.0 - alpha + 1e-15
    T = np.concatenate([np.ones_like(s[:, :1]), np.cumprod(s, axis=1)[:, :-1]], axis=1)
    return delta, alpha, s, T, alpha * T, e


def sample_pdf(bins, weights, u):
    """bins [N, B], weights [N, B - 1], u [N, U] -> [N, U]"""
    w = f64(weights) + 1e-5
    pdf = w / w.sum(axis=1, keepdims=True)
    cdf = np.concatenate([np.zeros_like(pdf[:, :1]), np.cumsum(pdf, axis=1)], axis=1)
    out = np.empty_like(f64(u))
    for n in range(cdf.shape[0]):
        inds = np.searchsorted(cdf[n], u[n], side="right")
        below, above = np.maximum(inds - 1, 0), np.minimum(inds, cdf.shape[1] - 1)
        denom = cdf[n, above] - cdf[n, below]
        denom = np.where(denom < 1e-5, 1.0, denom)
        t = (u[n] - cdf[n, below]) / denom
        out[n] = bins[n, below] + t * (bins[n, above] - bins[n, below])
    return out


def deterministic_u(N, U):
    return np.broadcast_to(np.linspace(0.5 / U, 1.0 - 0.5 / U, U), (N, U)).copy()


def upsample(z, sigma, nears, fars, scale, u, U, rays_o, rays_d, aabb):
    """new_z [N, U], new_xyz [N, U, 3], z_sorted [N, K], order [N, K]; u None: the deterministic row"""
    z = f64(z)
    N, S = z.shape
    delta, _, _, _, w, _ = alpha_weights(z, sigma, nears, fars, scale, S)
    z_mid = z[:, :-1] + 0.5 * delta[:, :-1]
    new_z = sample_pdf(z_mid, w[:, 1:-1], deterministic_u(N, U) if u is None else f64(u))
    both = np.concatenate([z, new_z], axis=1)
    order = np.argsort(both, axis=1, kind="stable")
    return new_z, points(rays_o, rays_d, new_z, aabb), np.take_along_axis(both, order, axis=1), order


def _columns(order, N, K):
    return np.broadcast_to(np.arange(K), (N, K)) if order is None else np.asarray(order, dtype=np.int64)


def weights(z_sorted, order, sigma_cat, nears, fars, scale, S):
    """weights and mask [N, K] in concatenated order"""
    z = f64(z_sorted)
    N, K = z.shape
    col = _columns(order, N, K)
    _, _, _, _, w, _ = alpha_weights(z, np.take_along_axis(f64(sigma_cat), col, axis=1), nears, fars, scale, S)
    out = np.empty_like(w)
    np.put_along_axis(out, col, w, axis=1)
    return out, out > 1e-4


def znorm(z_sorted, nears, fars):
    """clamp((z - near) / (far - near), 0, 1); a miss (near = far) is 0 / 0 = NaN and stays NaN"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.clip((f64(z_sorted) - f64(nears)[:, None]) / (f64(fars) - f64(nears))[:, None], 0.0, 1.0)


def composite(weights_cat, rgbs, z_sorted, order, nears, fars):
    """weights_sum [N], depth [N], image [N, 3]"""
    w, N, K = f64(weights_cat), z_sorted.shape[0], z_sorted.shape[1]
    w_sorted = np.take_along_axis(w, _columns(order, N, K), axis=1)
    return w.sum(axis=1), (w_sorted * znorm(z_sorted, nears, fars)).sum(axis=1), (w[:, :, None] * f64(rgbs)).sum(axis=1)


def composite_backward(grad_image, grad_weights_sum, grad_depth, sigma_cat, rgbs, z_sorted, order, nears, fars, scale, S):
    """grad_sigma_cat [N, K], grad_rgbs [N, K, 3]; a gradient given as None is zero:
    grad_sigma_p = delta_p scale exp(-delta_p scale sigma_p) (G_p T_p - sum_{q > p} G_q w_q / s_p), grad_rgb_p = w_p grad_image"""
    z = f64(z_sorted)
    N, K = z.shape
    col = _columns(order, N, K)
    rgb_sorted = np.take_along_axis(f64(rgbs), col[:, :, None], axis=1)
    delta, _, s, T, w, e = alpha_weights(z, np.take_along_axis(f64(sigma_cat), col, axis=1), nears, fars, scale, S)
    G = np.zeros((N, K))
    if grad_image is not None:
        G = G + (rgb_sorted * f64(grad_image)[:, None, :]).sum(axis=2)
    if grad_weights_sum is not None:
        G = G + f64(grad_weights_sum)[:, None]
    if grad_depth is not None:
        G = G + f64(grad_depth)[:, None] * znorm(z, nears, fars)
    X = G * w
    later = np.cumsum(X[:, ::-1], axis=1)[:, ::-1] - X
    g_sigma = delta * scale * e * (G * T - later / s)
    g_rgb = w[:, :, None] * (np.zeros((N, 1, 3)) if grad_image is None else f64(grad_image)[:, None, :])
    out_sigma, out_rgb = np.empty_like(g_sigma), np.empty_like(g_rgb)
    np.put_along_axis(out_sigma, col, g_sigma, axis=1)
    np.put_along_axis(out_rgb, np.broadcast_to(col[:, :, None], g_rgb.shape), g_rgb, axis=1)
    return out_sigma, out_rgb


def render(rays_o, rays_d, aabb, min_near, S, U, scale, density, color, noise=None, u=None, bg_color=1.0):
    """the whole route: density(x [M, 3]) -> sigma [M]; color(x [M, 3], d [M, 3]) -> [M, 3]; colours only where the weight exceeds
    1e-4 (zero elsewhere).  u None: the deterministic row.  Returns image, depth, weights_sum."""
    N = rays_o.shape[0]
    nears, fars, z, xyz = coarse_samples(rays_o, rays_d, aabb, min_near, S, noise)
    sigma = density(xyz.reshape(-1, 3)).reshape(N, S)
    order = None
    if U > 0:
        new_z, new_xyz, z, order = upsample(z, sigma, nears, fars, scale, u, U, rays_o, rays_d, aabb)
        sigma = np.concatenate([sigma, density(new_xyz.reshape(-1, 3)).reshape(N, U)], axis=1)
        xyz = np.concatenate([xyz, new_xyz], axis=1)
    w, mask = weights(z, order, sigma, nears, fars, scale, S)
    dirs = np.broadcast_to(f64(rays_d)[:, None, :], xyz.shape)
    rgbs = color(xyz.reshape(-1, 3), dirs.reshape(-1, 3)).reshape(N, -1, 3) * mask[:, :, None]
    ws, depth, image = composite(w, rgbs, z, order, nears, fars)
    return image + (1.0 - ws)[:, None] * bg_color, depth, ws
