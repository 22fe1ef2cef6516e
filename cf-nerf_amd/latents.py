"""The latents of a launch: column order, draw order, netchunk layout and the one decision "which latents does this train launch
use, and in what shape" (``train_latents``: api.render_rays, api.NeRF_Flows.forward and train.Trainer ask here).  Host logic on torch only.

Layout.  One latent set is ``[K,4] = eps_rgb (3) | eps_alpha (1)``, fp32 (``pack``).  A launch reads one set, or one set PER ROW:
``[n,K,4]`` with a row for each of its n rays (ray launches) or n points (NeRF_Flows.forward), ``CFNERF_F_EPS_ROWS``.
Draws (RUN = run_nerf_uncertainty_NF.py, MOD = model/models.py), always from torch's CPU generator like the reference:
  * ``"launch"`` mode (default): ``t_rand [N,S]`` (RUN:524, only if the caller has none and ``perturb > 0``), then eps_alpha, then eps_rgb
    (MOD:234,246) - ONE pair for the launch.
  * ``"netchunk"`` mode: the reference draws a fresh pair per ``netchunk`` points (batchify, RUN:47-64,82) inside every ``chunk``-ray cut
    of batchify_rays (RUN:88-100).  Per cut: ``t_rand [n_c,S]``, then per network call of the cut eps_alpha, eps_rgb, then - if
    ``raw_noise_std > 0`` - the ``randn([n_c,S,K])`` that raw2outputs draws and never uses (RUN:434); then the next cut
    (``draw_train_randomness``).  Ray i gets the pair of the network call that evaluates its points (``netchunk_eps_rows``).
Explicit latents are one packed set ``[K,4]`` or per-netchunk pairs ``[C,K,4]`` in draw order; they mean the same in either mode.
"""
import torch

LATENT_DRAWS = ("launch", "netchunk")


def pack(eps_alpha, eps_rgb):
    """``eps_alpha [..,K,1]`` / ``eps_rgb [..,K,3]`` as ``[..,K,4]`` fp32, rgb then alpha; None when both are None.  Explicit latents are
    ``[K,1]`` / ``[K,3]`` (one set) or ``[C,K,1]`` / ``[C,K,3]`` (one pair per netchunk): anything else is refused."""
    if eps_alpha is None and eps_rgb is None:
        return None
    if eps_alpha is None or eps_rgb is None or eps_alpha.dim() != eps_rgb.dim() or eps_alpha.dim() not in (2, 3):
        raise ValueError("eps_alpha and eps_rgb go together: [K,1] / [K,3] (one set) or [C,K,1] / [C,K,3] (one pair per netchunk)")
    return torch.cat([eps_rgb, eps_alpha], -1).to(torch.float32)


def to_device(eps, device):
    """Latents on ``device``; host tensors through pinned memory, not blocking the host (a pageable copy would stall the launch queue)."""
    if eps.is_cuda or (torch.is_grad_enabled() and eps.requires_grad):      # (latents on the autograd graph: one differentiable copy)
        return eps.to(device)
    return eps.pin_memory().to(device, non_blocking=True)


def check_rows(eps, n, what, hint=" (per-netchunk latents go through netchunk_eps_rows)"):
    """True when ``eps`` holds one ``[K,4]`` row per ray / point (CFNERF_F_EPS_ROWS), False for one ``[K,4]`` set.  The kernels read row i
    for ray / point i, so a launch of ``n`` must be given exactly ``n`` rows."""
    if eps.dim() == 3 and eps.shape[0] != n:
        raise ValueError(f"latent rows for {eps.shape[0]} {what}, the launch has {n}{hint}")
    return eps.dim() == 3


def draw_pairs(n, K):
    """n latent pairs from torch's CPU generator, eps_alpha then eps_rgb per network call (MOD:234,246), as ``[n,K,4]``."""
    out = torch.empty(n, K, 4)
    for c in range(n):
        ea = torch.empty([K, 1]).normal_()
        out[c] = pack(ea, torch.empty([K, 3]).normal_())
    return out


def ray_cuts(N, chunk):
    """(first ray, rays) of every batchify_rays cut of an N-ray batch (RUN:88-100); ``chunk=None``: one cut."""
    step = N if not chunk else int(chunk)
    return [(r0, min(step, N - r0)) for r0 in range(0, N, max(step, 1))]


def network_calls(n_points, netchunk):
    """Network calls (= latent pairs) batchify makes for ``n_points`` points (RUN:47-64)."""
    return -(-int(n_points) // int(netchunk))


def netchunk_count(N, S, netchunk, chunk=None):
    """Latent pairs the reference draws for an N-ray train batch of S samples per ray: every ``chunk``-ray cut restarts batchify's count."""
    return sum(network_calls(n * S, netchunk) for _, n in ray_cuts(N, chunk))


def netchunk_row_index(N, S, netchunk, chunk=None, with_count=False):
    """The latent pair (in draw order) of every ray of an N-ray batch, a non-decreasing host index ``[N]``: ray i gets the latents of the
    network call that evaluates its points.  Needs ``netchunk % S == 0`` (see the refusal below)."""
    netchunk, S = int(netchunk), int(S)
    if netchunk % S:
        raise NotImplementedError(f"netchunk ({netchunk}) is not a multiple of the samples per ray ({S}): the reference then changes "
                                  f"latents in the middle of a ray, which per-ray latent rows cannot express")
    per = netchunk // S                          # rays of one network call
    idx, base = [], 0
    for _, n in ray_cuts(N, chunk):
        idx.append(base + torch.arange(n) // per)
        base += network_calls(n * S, netchunk)
    idx = torch.cat(idx) if idx else torch.zeros(0, dtype=torch.long)
    return (idx, base) if with_count else idx


def netchunk_eps_rows(eps_chunks, N, S, netchunk, chunk=None):
    """Expand per-netchunk latents ``eps_chunks [C,K,4]`` (in draw order) to ray rows ``[N,K,4]`` (``netchunk_row_index``)."""
    idx, base = netchunk_row_index(N, S, netchunk, chunk, with_count=True)
    if eps_chunks.shape[0] != base:
        raise ValueError(f"{eps_chunks.shape[0]} latent pairs given; N={N}, S={S}, netchunk={netchunk}, chunk={chunk} needs {base}")
    if torch.is_grad_enabled() and eps_chunks.requires_grad:
        return _PairsToRows.apply(eps_chunks, idx)
    return eps_chunks.index_select(0, idx.to(eps_chunks.device)).contiguous()


class _PairsToRows(torch.autograd.Function):
    """``netchunk_eps_rows`` for pairs that ask for a gradient: the same ``index_select``, with a deterministic adjoint.  The rows of a pair
    are one contiguous segment (``idx`` is non-decreasing), so d pairs[c] is a plain sum over the segment - torch's own backward of
    ``index_select`` adds with atomics on the GPU, and the latent gradient is bit-reproducible from the kernels up."""

    @staticmethod
    def forward(ctx, pairs, idx):
        ctx.counts = torch.bincount(idx, minlength=pairs.shape[0]).tolist()      # (idx is a host tensor: no device round trip)
        return pairs.index_select(0, idx.to(pairs.device)).contiguous()

    @staticmethod
    def backward(ctx, d_rows):
        return rows_to_pairs_sum(d_rows, ctx.counts), None


def rows_to_pairs_sum(rows, counts):
    """Sum rows ``[N,...]`` over consecutive segments of ``counts[c]`` rows each -> ``[C,...]``: the adjoint of pairs -> rows, in a fixed
    order and without atomics (``_PairsToRows.backward``, ``train.Trainer`` for the pairs' latent gradient).  ``counts``: a host list, e.g.
    ``torch.bincount(netchunk_row_index(...), minlength=C).tolist()``."""
    out, r0 = rows.new_zeros(len(counts), *rows.shape[1:]), 0
    for c, n in enumerate(counts):
        if n:
            out[c] = rows[r0:r0 + n].sum(0)
        r0 += n
    return out


def netchunk_eps_point_rows(eps_chunks, P, netchunk):
    """Per-netchunk latents ``[C,K,4]`` as one row per point ``[P,K,4]`` (batchify over P points, RUN:47-64): a point is a ray of one sample."""
    return netchunk_eps_rows(eps_chunks, int(P), 1, netchunk)


def draw_train_randomness(N, S, K, chunk, netchunk, perturb, raw_noise_std=0.):
    """The randomness of one reference train render of N rays in netchunk mode, in the reference's order (module docstring).
    Returns ``(t_rand [N,S] or None, eps_chunks [C,K,4])``."""
    tr, eps = [], []
    for _, n in ray_cuts(N, chunk):
        if perturb > 0.:
            tr.append(torch.rand([n, S]))
        eps.append(draw_pairs(network_calls(n * S, netchunk), K))
        if raw_noise_std > 0.:
            torch.randn([n, S, K])
    t_rand = (torch.cat(tr, 0) if tr else torch.zeros(0, S)) if perturb > 0. else None
    return t_rand, (torch.cat(eps, 0) if eps else torch.zeros(0, K, 4))


def train_latents(mode, explicit, *, N, S, K, netchunk, chunk=None, perturb=0., raw_noise_std=0., own_t_rand=True):
    """The latents of ONE train launch of N rays with S samples each (points mode: N points, S = 1): ``(t_rand | None, eps, pairs | None)``.

    ``explicit`` is None, one packed set ``[K,4]`` or packed per-netchunk pairs ``[C,K,4]`` (they stay on their device; draws are on the
    CPU).  ``eps`` is ``[K,4]`` (one set for the launch) or rows ``[N,K,4]`` with the ``pairs [C,K,4]`` behind them: explicit pairs mean
    rows and an explicit set one set in either mode; with nothing explicit ``"launch"`` draws one pair and ``"netchunk"`` the
    reference's ``draw_train_randomness``.  ``t_rand [N,S]`` is what the CPU generator yielded on the way, for a caller without one of its
    own: always in an implicit netchunk draw, otherwise only with ``own_t_rand=False`` (drawn BEFORE the pair, RUN:524 -> MOD:234)."""
    if mode not in LATENT_DRAWS:
        raise ValueError(f"latent_draws must be one of {LATENT_DRAWS}, got {mode!r}")
    if explicit is None and mode == "netchunk":
        t_rand, explicit = draw_train_randomness(N, S, K, chunk, netchunk, perturb, raw_noise_std)
    else:
        t_rand = torch.rand([N, S]) if perturb > 0. and not own_t_rand else None
        if explicit is None:
            explicit = draw_pairs(1, K)[0]
    if explicit.dim() == 2:
        return t_rand, explicit, None
    return t_rand, netchunk_eps_rows(explicit, N, S, netchunk, chunk), explicit
