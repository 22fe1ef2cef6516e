"""The yardstick of the ray regularisers (CFNERF_F_RAY_REG, include/cfnerf.h): plain torch, any dtype, any device.

* ``quadratic``: the DEFINITION - the [S,S] table of mip-NeRF 360's distortion loss and the ray entropy of INTEGRATION.md section 12 (c) -
  differentiable by autograd; O(S^2) per (ray, latent), for small shapes in fp64.
* ``closed_forms``: the O(S) closed forms in the Q/R arrangement with their hand-written gradients: in fp64 the
  reference the kernel is held to, in fp32 the "what plain torch gets" figure its error is compared with.
* the input makers the CPU and the GPU tests share."""
import torch


def _near_far(rays, z):
    """rays: None (s = z), (near, far) numbers, or a ray_batch [N,11] (columns 6, 7) -> near [N,1], span [N,1] in z's dtype, or (None, None)"""
    if rays is None:
        return None, None
    if isinstance(rays, (tuple, list)):
        near = torch.full_like(z[:, :1], float(rays[0]))
        far = torch.full_like(z[:, :1], float(rays[1]))
    else:
        near, far = rays[:, 6:7].to(z.dtype), rays[:, 7:8].to(z.dtype)
    return near, far - near


def geometry(z, rays):
    """s, m, delta [N,S] and the span [N,1] (1 without rays) of the intervals: the last sample is the point m = s, delta = 0"""
    near, span = _near_far(rays, z)
    s = z if near is None else (z - near) / span
    m = torch.cat([(s[:, 1:] + s[:, :-1]) / 2, s[:, -1:]], 1)
    dl = torch.cat([s[:, 1:] - s[:, :-1], torch.zeros_like(s[:, -1:])], 1)
    return s, m, dl, (torch.ones_like(z[:, :1]) if span is None else span)


def entropy_12c(w):
    """INTEGRATION.md section 12 (c), verbatim: [N,K]"""
    p = w / (w.sum(1, keepdim=True) + 1e-10)
    return -(p * torch.log(p + 1e-10)).sum(1)


def quadratic(w, z, rays=None, distortion=0., entropy=0., acc_min=0.1, n_total=None):
    """(reg, dist, ent, frac) by the definition; reg is differentiable in w and z.  The mask is a constant of the graph."""
    N, S, K = w.shape
    n = N if n_total is None else n_total
    _, m, dl, _ = geometry(z, rays)
    D = (w[:, :, None, :] * w[:, None, :, :] * (m[:, :, None] - m[:, None, :]).abs()[..., None]).sum((1, 2)) + (w * w * dl[..., None]).sum(1) / 3
    mask = (w.detach().sum(1) > acc_min).to(w.dtype)
    dist = D.sum() / (n * K)
    ent = (mask * entropy_12c(w)).sum() / (n * K)
    frac = mask.sum() / (n * K)
    return distortion * dist + entropy * ent, dist, ent, frac


def closed_forms(w, z, rays=None, distortion=0., entropy=0., acc_min=0.1, n_total=None):
    """{'scalars': [reg, dist, ent, frac], 'd_weights': [N,S,K], 'd_z': [N,S]} in the dtype of w: prefix / suffix sums along the ray, no [S,S] table.
    Q_i = sum_{j<i} W_<=j dm_j, R_i = sum_{j>=i} W_>j dm_j (dm_j = m_j+1 - m_j): D = 2 sum w Q + 1/3 sum w^2 delta, dD/dw = 2 (Q + R) + 2/3 w delta."""
    N, S, K = w.shape
    n = N if n_total is None else n_total
    _, m, dl, span = geometry(z, rays)
    m, dl = m[..., None], dl[..., None]
    dm = torch.cat([m[:, 1:] - m[:, :-1], torch.zeros_like(m[:, :1])], 1)
    Wi = torch.cumsum(w, 1)                                                        # W_<=i
    zero = torch.zeros_like(w[:, :1])
    Wlt = torch.cat([zero, Wi[:, :-1]], 1)                                         # W_<i
    Wsuf = torch.cat([torch.flip(torch.cumsum(torch.flip(w, [1]), 1), [1])[:, 1:], zero], 1)      # W_>i, summed from the back: no A - W_<=i
    Q = torch.cat([zero, torch.cumsum(Wi * dm, 1)[:, :-1]], 1)
    R = torch.flip(torch.cumsum(torch.flip(Wsuf * dm, [1]), 1), [1])
    D = (2 * w * Q).sum(1) + (w * w * dl).sum(1) / 3
    gD = 2 * (Q + R) + 2 * w * dl / 3
    dmm = (2 * w * (Wlt - Wsuf)).sum(-1)                                      # dD/dm_i, dD/ddelta_i over K
    dd = (w * w / 3).sum(-1)
    gs = torch.zeros_like(z)
    gs[:, :-1] += dmm[:, :-1] / 2 - dd[:, :-1]
    gs[:, 1:] += dmm[:, :-1] / 2 + dd[:, :-1]
    gs[:, -1] += dmm[:, -1]
    A = w.sum(1, keepdim=True)
    p = w / (A + 1e-10)
    g = -torch.log(p + 1e-10) - p / (p + 1e-10)
    mask = (A > acc_min).to(w.dtype)
    H = entropy_12c(w)
    gH = mask * (g - (p * g).sum(1, keepdim=True)) / (A + 1e-10)
    dist = D.sum() / (n * K)
    ent = (mask[:, 0] * H).sum() / (n * K)
    frac = mask.sum() / (n * K)
    return {"scalars": torch.stack([distortion * dist + entropy * ent, dist, ent, frac]),
            "d_weights": (distortion * gD + entropy * gH) / (n * K),
            "d_z": distortion * gs / span / (n * K),
            "A": A[:, 0]}


def mask_margin(w64, acc_min):
    """min |A - acc_min| over the (ray, latent) pairs, on the fp64 side: below ~1e-3 fp32 and fp64 may disagree on the mask"""
    return (w64.sum(1) - acc_min).abs().min().item()


# ---------------------------------------------------------------- inputs
def composite_weights(N, S, K, seed, lo=2., hi=6., tie=None):
    """weights [N,S,K] composited from a random raw as raw2outputs does (RUN:424-443) over sorted random depths in [lo, hi]; fp64"""
    g = torch.Generator().manual_seed(seed)
    z = torch.sort(torch.rand(N, S, dtype=torch.float64, generator=g) * (hi - lo) + lo, 1)[0]
    if tie is not None and S > tie + 1:
        z[:, tie + 1] = z[:, tie]
    raw = torch.randn(N, S, K, dtype=torch.float64, generator=g) * 2
    d = torch.cat([z[:, 1:] - z[:, :-1], torch.full((N, 1), 1e10, dtype=torch.float64)], 1)
    a = 1 - torch.exp(-torch.nn.functional.softplus(raw) * d[..., None])
    T = torch.cumprod(torch.cat([torch.ones(N, 1, K, dtype=torch.float64), 1 - a + 1e-10], 1), 1)[:, :-1]
    return a * T, z


def peaked_weights(N, S, K, seed):
    """the "surface" case: three neighbouring samples carry 0.99 of every ray, 1e-6 elsewhere; depths sorted in [0, 1]; fp64"""
    g = torch.Generator().manual_seed(seed)
    z = torch.sort(torch.rand(N, S, dtype=torch.float64, generator=g), 1)[0]
    w = torch.full((N, S, K), 1e-6, dtype=torch.float64)
    c = torch.randint(S // 2, S - 10, (N,), generator=g)
    for n in range(N):
        w[n, c[n] - 1] = 0.3
        w[n, c[n]] = 0.5
        w[n, c[n] + 1] = 0.19
    return w, z


def rel_err(got, ref):
    """max abs error over the largest reference entry"""
    return ((got.double().cpu() - ref.double().cpu()).abs().max() / ref.double().abs().max().clamp_min(1e-300)).item()
