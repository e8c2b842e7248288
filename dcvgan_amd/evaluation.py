"""On-device evaluation: Inception score, Fréchet distance and kernel distance.

The reference's ``Trainer.evaluate`` (trainer.py:171-224) generates ``eval_num_samples`` clips, moves the generators to the CPU, writes every clip
as an mp4 and lets an external package read the files back for IS / FID / PRD.  Here the clips and their features stay in device memory.  The feature network is the
caller's, handed over as a callable; everything after it is this module's:

* ``FeatureMoments``: streaming mean and covariance of the features (``dcv_eval_moments_update``: fp32 features, fp64 sums on the fp64 matrix pipe),
* ``InceptionStats``: the sums the Inception score is finalised from (``dcv_eval_inception_update``: an fp64 softmax per row),
* ``kernel_distance``: KID with the cubic polynomial kernel over drawn subsets (``dcv_eval_kid_draw`` + ``dcv_eval_kid_sums``; the m x m kernel matrices are never
  written),
* ``manifold_metrics``: improved precision / recall and density / coverage (``dcv_eval_row_norms``, ``dcv_eval_knn_radii``, ``dcv_eval_manifold_counts``,
  ``dcv_eval_manifold_reduce``; the n x n distance matrices are never written), with ``manifold_host`` as its numpy mirror,
* ``prd_metrics``: PRD, the reference's third metric (R runs of k-means over the union of the two feature sets — ``dcv_eval_prd_seed``,
  ``dcv_eval_prd_assign``, ``dcv_eval_prd_update``, ``dcv_eval_prd_count`` — then the precision-recall curve of the cluster histograms in host numpy), with
  ``prd_host`` as its numpy mirror,
* ``frechet_distance``: the O(D^3) eigenvalue step on the host in numpy — it runs once per evaluation and produces a number for the host's logger anyway,
* ``Evaluator``: generator -> extractor -> statistics without a clip or a feature crossing PCIe.

Every accumulation has one fixed order and no floating-point atomic: the same sequence of calls gives the same bits.  ``draw_host`` is an integer-exact numpy mirror
of the subset draw, as ``clipstore.permute_host`` is of the epoch shuffle: the specification the kernel is tested against.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import clipstore
from . import native as N
from .native import NativeError, check, lib, ptr, stream_ptr

MAX_DIM = 4096                       # features per row (D) and classes per row (K): the kernels' limit
MAX_SUBSETS, MAX_SUBSET_SIZE = 4096, 65536
KID_SALT = 0x9FB21C651E98DF25        # DCV_EVAL_KID_SALT: the draw's Philox key is the seed plus this constant
_M64 = 0xFFFFFFFFFFFFFFFF
METRICS = ("is", "fid", "kid", "pr", "dc", "prcurve")
DEFAULT_METRICS = ("is", "fid", "kid")
MAX_K, MAX_COL_SPLITS = 16, 64        # neighbours and column shares of the k-nearest-neighbour metrics: the kernels' limits
PRD_SALT = 0xC2B2AE3D27D4EB4F        # DCV_EVAL_PRD_SALT: the seeding's Philox key is the seed plus this constant
PRD_MAX_CLUSTERS, PRD_MAX_RUNS, PRD_MAX_ITERS, PRD_MAX_ROW_SPLITS = 64, 64, 1000, 64      # PRD's k-means: the kernels' limits, and the Lloyd iterations of one call

_STATS = {"launches": 0}


def launches() -> int:
    """Kernel launches this module has issued so far, in this process (dcv_eval_inception_update, dcv_eval_kid_sums, dcv_eval_knn_radii, dcv_eval_manifold_counts
    and dcv_eval_prd_assign are two each, dcv_eval_prd_update is three, every other entry one)."""
    return _STATS["launches"]


def _call(name: str, n_launches: int, *args):
    check(getattr(lib(), name)(*args), name)
    _STATS["launches"] += n_launches


def _device(device) -> torch.device:
    from . import util
    return torch.device(device if device is not None else util.current_device())


def _rows(t, width: Optional[int], what: str) -> Tuple[int, int, int]:
    """(n, width, row stride in elements) of a (n, width) fp32 device tensor whose rows are dense; a row-strided view is taken as it is, anything else is refused."""
    if not isinstance(t, torch.Tensor):
        raise NativeError(f"{what}: expected a tensor, got {type(t).__name__}")
    N._require(t, what)
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1 or (width is not None and t.shape[1] != width):
        raise NativeError(f"{what}: expected a (n, {width if width is not None else 'D'}) tensor with n >= 1, got {tuple(t.shape)}")
    n, w = int(t.shape[0]), int(t.shape[1])
    if w > MAX_DIM or n >= 2 ** 31:
        raise NativeError(f"{what}: at most {MAX_DIM} values per row and fewer than 2^31 rows, got {tuple(t.shape)}")
    stride = int(t.stride(0)) if n > 1 else w
    if (w > 1 and t.stride(1) != 1) or stride < w:
        raise NativeError(f"{what}: rows must be dense and at least a row apart (a row-strided view is fine), got strides {tuple(t.stride())} for shape {tuple(t.shape)}")
    return n, w, stride


_ZERO_ROW = 1024      # fp32 words of the zero row a state is cleared from; a state buffer is a whole number of such rows (512 doubles)
_ZEROS = {}


def _state_buffer(n_doubles: int, device) -> torch.Tensor:
    """One flat fp64 buffer for an additive state and, in its last used slot, the row count during a collective: zeros, padded to whole zero rows.  A host tensor
    copied over once (no kernel)."""
    padded = -(-int(n_doubles) // (_ZERO_ROW // 2)) * (_ZERO_ROW // 2)
    return torch.zeros((padded,), dtype=torch.float64).to(device)


def _clear(buf: torch.Tensor) -> None:
    """buf <- 0 on the device by the library's strided copy (dcv_axpby, one launch) of a zero row broadcast over the buffer's rows — a copy, not a scaling, so a NaN
    left by an earlier stream does not survive; on the host torch's fill."""
    if not buf.is_cuda:
        buf.zero_()
        return
    from . import ops
    key = str(buf.device)
    if key not in _ZEROS:
        _ZEROS[key] = torch.zeros(_ZERO_ROW, dtype=torch.float32).to(buf.device)
    rows = buf.numel() * 2 // _ZERO_ROW
    ops._axpby(_ZEROS[key].view(1, 1, 1, 1, _ZERO_ROW).expand(1, rows, 1, 1, _ZERO_ROW), 1.0, None, 0.0, buf.view(torch.float32).view(1, rows, 1, 1, _ZERO_ROW))
    _STATS["launches"] += 1


def _dist_world(group=None) -> int:
    import torch.distributed as dist
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


def _all_reduce_state(buf: torch.Tensor, used: int, n: int, group=None) -> int:
    """ONE collective (SUM) over the state and its row count: the count rides in slot `used` of the state's own buffer as a double (exact below 2^53), so the
    collective runs on the tensor's device — a backend registered for device tensors alone, as nccl is, serves it — and cannot leave the sums reduced and the count
    not.  -> the summed count; the slot is zero again afterwards."""
    import torch.distributed as dist
    slot = buf[used:used + 1]
    slot.copy_(torch.tensor([float(n)], dtype=torch.float64))      # host -> device copy, no kernel
    dist.all_reduce(buf[:used + 1], op=dist.ReduceOp.SUM, group=group)
    total = int(round(float(slot.cpu().item())))
    slot.copy_(torch.zeros(1, dtype=torch.float64))
    return total


# --------------------------------------------------------------------------- #
# feature moments and the Fréchet distance
# --------------------------------------------------------------------------- #
class FeatureMoments:
    """``FeatureMoments(dim, device=None)``: the additive state ``(n, sum, gram)`` of a stream of ``dim``-dimensional features — ``sum`` (dim,) and ``gram`` (dim, dim)
    fp64 in device memory, the row count on the host, where it is known.  ``update(feats)`` is one launch and no host read; ``mean()`` / ``cov()`` read the state
    back (host fp64).  On ``device="cpu"`` the object only holds statistics (``load``, ``load_state_dict``): updating it is refused."""

    def __init__(self, dim: int, device=None):
        if not 1 <= int(dim) <= MAX_DIM:
            raise ValueError(f"FeatureMoments: 1 <= dim <= {MAX_DIM}, got {dim!r}")
        self.dim, self.device, self.n = int(dim), _device(device), 0
        D = self.dim
        self._buf = _state_buffer(D * D + D + 1, self.device)      # gram, sum, and the slot the row count rides in during all_reduce
        self.gram, self.sum = self._buf[:D * D].view(D, D), self._buf[D * D:D * D + D]

    def reset(self) -> "FeatureMoments":
        """Back to no rows: the device state is cleared in place (one launch), nothing is allocated or copied from the host."""
        _clear(self._buf)
        self.n = 0
        return self

    def update(self, feats: torch.Tensor) -> "FeatureMoments":
        """sum += sum_i x_i, gram += X^T X for a (n, dim) fp32 device tensor (a row-strided view is passed as it is)."""
        n, _, stride = _rows(feats, self.dim, "FeatureMoments.update")
        if not self.sum.is_cuda:
            raise NativeError(f"FeatureMoments: the state is on {self.sum.device} — the moments are accumulated on the GPU only (there is no CPU fallback)")
        if self.n + n >= 2 ** 53:
            raise NativeError("FeatureMoments: row count out of range")
        _call("dcv_eval_moments_update", 1, ptr(feats), n, self.dim, stride, ptr(self.sum), ptr(self.gram), stream_ptr())
        self.n += n
        return self

    # ---- host reads ----------------------------------------------------------------------------------------------------------------------------------------
    def _host(self):
        return self.sum.cpu().numpy().astype(np.float64), self.gram.cpu().numpy().astype(np.float64)

    def mean(self) -> np.ndarray:
        if self.n < 1:
            raise ValueError("FeatureMoments.mean: no rows yet")
        return self._host()[0] / float(self.n)

    def cov(self) -> np.ndarray:
        """The unbiased covariance (gram - s s^T / n) / (n - 1), as numpy.cov(rowvar=False) has it."""
        if self.n < 2:
            raise ValueError(f"FeatureMoments.cov: at least two rows are needed, got {self.n}")
        s, g = self._host()
        return (g - np.outer(s, s) / float(self.n)) / float(self.n - 1)

    def state_dict(self):
        s, g = self._host()
        return dict(dim=self.dim, n=int(self.n), sum=s, gram=g)

    def load_state_dict(self, sd) -> "FeatureMoments":
        s, g = np.asarray(sd["sum"], dtype=np.float64), np.asarray(sd["gram"], dtype=np.float64)
        if int(sd["dim"]) != self.dim or s.shape != (self.dim,) or g.shape != (self.dim, self.dim) or int(sd["n"]) < 0:
            raise ValueError(f"FeatureMoments: built for dim {self.dim}, the state has dim {sd['dim']}, sum {s.shape}, gram {g.shape}, n {sd['n']}")
        self.sum.copy_(torch.from_numpy(np.ascontiguousarray(s)))
        self.gram.copy_(torch.from_numpy(np.ascontiguousarray(g)))
        self.n = int(sd["n"])
        return self

    def save(self, path) -> None:
        """An .npz with ``mu``, ``sigma``, ``n``: the usual shape of precomputed real statistics."""
        np.savez(path, mu=self.mean(), sigma=self.cov(), n=np.int64(self.n))

    @classmethod
    def load(cls, path, device=None) -> "FeatureMoments":
        """The moments of a saved ``mu`` / ``sigma`` / ``n``: sum = n mu, gram = (n - 1) sigma + n mu mu^T."""
        with np.load(path) as z:
            mu, sigma, n = np.asarray(z["mu"], dtype=np.float64), np.asarray(z["sigma"], dtype=np.float64), int(z["n"])
        if mu.ndim != 1 or sigma.shape != (mu.size, mu.size) or n < 2:
            raise ValueError(f"FeatureMoments.load: mu {mu.shape}, sigma {sigma.shape}, n {n}")
        fm = cls(mu.size, device)
        return fm.load_state_dict(dict(dim=mu.size, n=n, sum=n * mu, gram=(n - 1) * sigma + n * np.outer(mu, mu)))

    def all_reduce(self, group=None) -> "FeatureMoments":
        """The state is additive: SUM over ``sum``, ``gram`` and ``n`` of every rank, in one collective on the state's device tensor (a collective call; nothing to
        do in a single process)."""
        if _dist_world(group) > 1:
            self.n = _all_reduce_state(self._buf, self.dim * self.dim + self.dim, self.n, group)
        return self


def frechet_distance(a: FeatureMoments, b: FeatureMoments) -> float:
    """|mu_a - mu_b|^2 + tr S_a + tr S_b - 2 tr (S_a^1/2 S_b S_a^1/2)^1/2 (Heusel et al. 2017) in host fp64, from symmetric eigendecompositions alone.

    With S_a = V diag(w) V^T (``eigh``, w clipped at 0) and R = S_a^1/2 = V diag(sqrt w) V^T, the trace term is sum_i sqrt(max(lambda_i, 0)) over
    lambda = eigvalsh(R S_b R).  R S_b R = V M V^T with M = diag(sqrt w) (V^T S_b V) diag(sqrt w), so lambda is taken from M, restricted to the directions in which
    S_a is numerically non-zero (w_i > dim * eps * max w; the others are the clipped ones and rounding noise around them): the same non-zero eigenvalues.  The
    restriction matters for a rank-deficient S_a (fewer rows than features): a symmetric eigensolver returns the zero eigenvalues of the full matrix as
    +-eps |M|, whose square roots, 1e-8 |S| each, are the error the sqrtm formulation shows there.  For the same reason a lambda_i below len(lambda) * eps * max lambda
    (S_b deficient inside the range of S_a) is the solver's noise around zero and counts as zero."""
    if not isinstance(a, FeatureMoments) or not isinstance(b, FeatureMoments):
        raise TypeError("frechet_distance: two FeatureMoments")
    if a.dim != b.dim:
        raise ValueError(f"frechet_distance: feature dimensions {a.dim} and {b.dim}")
    mu_a, mu_b, sa, sb = a.mean(), b.mean(), a.cov(), b.cov()
    w, v = np.linalg.eigh((sa + sa.T) * 0.5)
    keep = w > a.dim * np.finfo(np.float64).eps * max(float(w.max()), 0.0)
    r, v = np.sqrt(w[keep]), v[:, keep]
    m = (v.T @ ((sb + sb.T) * 0.5) @ v) * r[:, None] * r[None, :]
    lam = np.linalg.eigvalsh((m + m.T) * 0.5) if m.size else np.zeros(0)
    if lam.size:
        lam = np.where(lam > lam.size * np.finfo(np.float64).eps * max(float(lam.max()), 0.0), lam, 0.0)
    d = mu_a - mu_b
    return float(d @ d + np.trace(sa) + np.trace(sb) - 2.0 * np.sum(np.sqrt(lam)))


# --------------------------------------------------------------------------- #
# the Inception score
# --------------------------------------------------------------------------- #
def inception_score_from_state(state, n: int) -> float:
    """exp(state[K] / n - sum_k pbar_k log pbar_k), pbar = state[:K] / n (Salimans et al. 2016: exp of the mean KL(p(y|x) || p(y))); a class with pbar = 0 adds
    nothing."""
    state = np.asarray(state, dtype=np.float64).reshape(-1)
    if int(n) < 1 or state.size < 2:
        raise ValueError(f"inception score: at least one row and one class, got n {n}, state of {state.size}")
    pbar = state[:-1] / float(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        marginal = np.where(pbar == 0.0, 0.0, pbar * np.log(pbar))
    return float(np.exp(state[-1] / float(n) - marginal.sum()))


class InceptionStats:
    """``InceptionStats(num_classes, device=None)``: ``state[k] = sum_i p_ik``, ``state[K] = sum_i sum_k p_ik log p_ik`` as K + 1 doubles in device memory;
    ``update(logits)`` is two launches and no host read, ``score()`` finalises on the host."""

    def __init__(self, num_classes: int, device=None):
        if not 1 <= int(num_classes) <= MAX_DIM:
            raise ValueError(f"InceptionStats: 1 <= num_classes <= {MAX_DIM}, got {num_classes!r}")
        self.num_classes, self.device, self.n = int(num_classes), _device(device), 0
        self._buf = _state_buffer(self.num_classes + 2, self.device)      # the K + 1 sums, and the slot the row count rides in during all_reduce
        self.state = self._buf[:self.num_classes + 1]

    def reset(self) -> "InceptionStats":
        """Back to no rows: the device state is cleared in place (one launch)."""
        _clear(self._buf)
        self.n = 0
        return self

    def update(self, logits: torch.Tensor) -> "InceptionStats":
        n, K, stride = _rows(logits, self.num_classes, "InceptionStats.update")
        if not self.state.is_cuda:
            raise NativeError(f"InceptionStats: the state is on {self.state.device} — the sums are accumulated on the GPU only (there is no CPU fallback)")
        need = int(lib().dcv_eval_inception_workspace_bytes(n, K))
        ws = N.scratch.get("eval_inception", need, logits.device)
        _call("dcv_eval_inception_update", 2, ptr(logits), n, K, stride, ptr(self.state), ptr(ws), ws.numel(), stream_ptr())
        self.n += n
        return self

    def state_host(self) -> np.ndarray:
        return self.state.cpu().numpy().astype(np.float64)

    def score(self) -> float:
        return inception_score_from_state(self.state_host(), self.n)

    def state_dict(self):
        return dict(num_classes=self.num_classes, n=int(self.n), state=self.state_host())

    def load_state_dict(self, sd) -> "InceptionStats":
        s = np.asarray(sd["state"], dtype=np.float64)
        if int(sd["num_classes"]) != self.num_classes or s.shape != (self.num_classes + 1,):
            raise ValueError(f"InceptionStats: built for {self.num_classes} classes, the state has {sd['num_classes']} and shape {s.shape}")
        self.state.copy_(torch.from_numpy(np.ascontiguousarray(s)))
        self.n = int(sd["n"])
        return self

    def all_reduce(self, group=None) -> "InceptionStats":
        if _dist_world(group) > 1:
            self.n = _all_reduce_state(self._buf, self.num_classes + 1, self.n, group)
        return self


# --------------------------------------------------------------------------- #
# the kernel distance
# --------------------------------------------------------------------------- #
def draw_host(seed: int, subsets: int, m: int, na: int, nb: int) -> np.ndarray:
    """The (subsets, 2, m) int32 table dcv_eval_kid_draw writes — integers only, the specification of the kernel.  table[s][side][i] = perm(i): the clip store's
    keyed bijection (8 Feistel rounds over Philox4x32-10, cycle-walked) on [0, na) for side 0 and [0, nb) for side 1, with key = seed + KID_SALT and the Philox
    counter {R, r, s, side} in round r."""
    subsets, m, na, nb = int(subsets), int(m), int(na), int(nb)
    if not (1 <= subsets <= MAX_SUBSETS and 2 <= m <= MAX_SUBSET_SIZE and m <= na < 2 ** 31 and m <= nb < 2 ** 31):
        raise ValueError(f"draw_host: 1 <= subsets <= {MAX_SUBSETS}, 2 <= m <= {MAX_SUBSET_SIZE}, m <= na, nb < 2^31; got {subsets}, {m}, {na}, {nb}")
    key = (int(seed) + KID_SALT) & _M64
    k0, k1 = key & 0xFFFFFFFF, key >> 32
    out = np.empty((subsets, 2, m), dtype=np.int32)
    s_col = np.repeat(np.arange(subsets, dtype=np.uint64), m)
    for side, n_rows in ((0, na), (1, nb)):
        h = clipstore.half_bits(n_rows)
        mask = np.uint64((1 << h) - 1)
        x = np.tile(np.arange(m, dtype=np.uint64), subsets)
        todo = np.ones(x.shape, dtype=bool)
        while todo.any():      # cycle walking: only the values still outside [0, n_rows) go round again
            v = x[todo]
            L, R = v >> np.uint64(h), v & mask
            for r in range(clipstore.FEISTEL_ROUNDS):
                f = clipstore.philox4x32_10(R, r, s_col[todo], side, k0, k1)[0] & mask
                L, R = R, L ^ f
            v = (L << np.uint64(h)) | R
            x[todo] = v
            todo[todo] = v >= np.uint64(n_rows)
        out[:, side, :] = x.reshape(subsets, m).astype(np.int32)
    return out


def mmd2_from_sums(out, m: int) -> np.ndarray:
    """MMD^2_s = out0 / (m (m - 1)) + out1 / (m (m - 1)) - 2 out2 / m^2 per subset: the unbiased estimator of Binkowski et al. 2018."""
    o = np.asarray(out, dtype=np.float64).reshape(-1, 3)
    m = float(m)
    return o[:, 0] / (m * (m - 1.0)) + o[:, 1] / (m * (m - 1.0)) - 2.0 * o[:, 2] / (m * m)


def kid_sums(fa: torch.Tensor, fb: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """The (subsets, 3) fp64 device tensor dcv_eval_kid_sums writes for a contiguous (subsets, 2, m) int32 device table: per subset the sums of
    k(x, y) = (x.y / D + 1)^3 over i != j of the a rows, of the b rows, and over all (i, j) across.  Two launches, no host read.  The table's entries are the
    caller's to keep inside [0, na) x [0, nb) (kernel_distance checks an injected one; a row named outside counts as NaN, nothing is read for it)."""
    na, D, sa = _rows(fa, None, "kernel distance: features a")
    nb, _, sb = _rows(fb, D, "kernel distance: features b")
    if not isinstance(table, torch.Tensor) or not table.is_cuda or table.dtype != torch.int32 or table.dim() != 3 or table.shape[1] != 2 or not table.is_contiguous() \
            or not 1 <= table.shape[0] <= MAX_SUBSETS or not 2 <= table.shape[2] <= MAX_SUBSET_SIZE:
        got = f"{table.dtype}{tuple(table.shape)} on {table.device}" if isinstance(table, torch.Tensor) else type(table).__name__
        raise NativeError(f"kernel distance: expected a contiguous (subsets <= {MAX_SUBSETS}, 2, 2 <= m <= {MAX_SUBSET_SIZE}) int32 device table, got {got}")
    subsets, m = int(table.shape[0]), int(table.shape[2])
    need = int(lib().dcv_eval_kid_workspace_bytes(subsets, m))
    ws = N.scratch.get("eval_kid", need, fa.device)
    out = torch.empty((subsets, 3), dtype=torch.float64, device=fa.device)
    _call("dcv_eval_kid_sums", 2, ptr(fa), sa, na, ptr(fb), sb, nb, D, ptr(table), subsets, m, ptr(ws), ws.numel(), ptr(out), stream_ptr())
    return out


def kid_draw(na: int, nb: int, subsets: int, m: int, seed: int, device) -> torch.Tensor:
    """The (subsets, 2, m) int32 device table of draw_host: one launch."""
    table = torch.empty((int(subsets), 2, int(m)), dtype=torch.int32, device=device)
    _call("dcv_eval_kid_draw", 1, ptr(table), int(subsets), int(m), int(na), int(nb), int(seed) & _M64, stream_ptr())
    return table


def kernel_distance(fa: torch.Tensor, fb: torch.Tensor, num_subsets: int = 100, subset_size: int = 1000, seed: int = 0,
                    table: Optional[torch.Tensor] = None) -> Tuple[float, float]:
    """(mean, std) over the subsets of MMD^2 between the rows of ``fa`` (na, D) and ``fb`` (nb, D), fp32 device tensors, with the kernel (x.y / D + 1)^3 and
    m = min(subset_size, na, nb) rows of each per subset.  The defaults are those of Karras et al. 2020 (100 subsets of 1000); std is the population standard
    deviation of the per-subset estimates.  ``table``: an explicit (subsets, 2, m) int32 device table instead of the draw (read back and checked here)."""
    na, D, _ = _rows(fa, None, "kernel distance: features a")
    nb, _, _ = _rows(fb, D, "kernel distance: features b")
    if table is None:
        m = min(int(subset_size), na, nb)
        if not 1 <= int(num_subsets) <= MAX_SUBSETS or not 2 <= m <= MAX_SUBSET_SIZE:
            raise NativeError(f"kernel distance: 1 <= num_subsets <= {MAX_SUBSETS} and 2 <= min(subset_size, na, nb) <= {MAX_SUBSET_SIZE}; got {num_subsets} subsets, "
                              f"subset_size {subset_size}, na {na}, nb {nb}")
        table = kid_draw(na, nb, int(num_subsets), m, seed, fa.device)
    else:
        if not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or table.dim() != 3 or table.shape[1] != 2:
            raise NativeError("kernel distance: the table must be a (subsets, 2, m) int32 device tensor")
        rows = table.cpu().numpy()
        if rows.size and (rows.min() < 0 or rows[:, 0].max() >= na or rows[:, 1].max() >= nb):
            raise ValueError(f"kernel distance: the table names rows outside [0, {na}) x [0, {nb})")
    out = kid_sums(fa, fb, table)
    mmd2 = mmd2_from_sums(out.cpu().numpy(), int(table.shape[2]))
    return float(mmd2.mean()), float(mmd2.std())


# --------------------------------------------------------------------------- #
# precision / recall and density / coverage
# --------------------------------------------------------------------------- #
def _k(k, what: str) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_K:
        raise ValueError(f"{what}: 1 <= k <= {MAX_K}, got {k!r}")
    return int(k)


def _splits(col_splits, what: str) -> int:
    if isinstance(col_splits, bool) or not isinstance(col_splits, (int, np.integer)) or not 0 <= int(col_splits) <= MAX_COL_SPLITS:
        raise ValueError(f"{what}: 0 <= col_splits <= {MAX_COL_SPLITS} (0: the library chooses), got {col_splits!r}")
    return int(col_splits)


def _vector(t, n: int, dtype, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or t.dim() != 1 or t.shape[0] != n or not t.is_contiguous():
        got = f"{t.dtype}{tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise NativeError(f"{what}: expected a contiguous ({n},) {dtype} device tensor, got {got}")
    return t


def row_norms(feats: torch.Tensor) -> torch.Tensor:
    """The (n,) fp64 device tensor of ``|x_i|^2 = sum_d x[i][d]^2`` (features ascending) for a (n, D) fp32 device tensor.  One launch."""
    n, D, stride = _rows(feats, None, "row_norms")
    out = torch.empty((n,), dtype=torch.float64, device=feats.device)
    _call("dcv_eval_row_norms", 1, ptr(feats), n, D, stride, ptr(out), stream_ptr())
    return out


def knn_radii(feats: torch.Tensor, k: int, col_splits: int = 0, norms: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The (n,) fp64 device tensor ``rad2[i]`` = the k-th smallest ``d2(x_i, x_j)`` over ``j != i`` (self excluded by index, a NaN distance never selected; +inf where
    fewer than k distances survive).  ``norms``: ``row_norms(feats)`` if the caller has them already.  Two launches (three without ``norms``), no host read; the result
    is the same bits for every ``col_splits``."""
    n, D, stride = _rows(feats, None, "knn_radii")
    k, col_splits = _k(k, "knn_radii"), _splits(col_splits, "knn_radii")
    if n < k + 1:
        raise NativeError(f"knn_radii: the {k}-th neighbour needs at least {k + 1} rows, got {n}")
    norms = row_norms(feats) if norms is None else _vector(norms, n, torch.float64, "knn_radii: norms")
    need = int(lib().dcv_eval_knn_workspace_bytes(n, k, col_splits))
    ws = N.scratch.get("eval_knn", need, feats.device)
    out = torch.empty((n,), dtype=torch.float64, device=feats.device)
    _call("dcv_eval_knn_radii", 2, ptr(feats), n, D, stride, ptr(norms), k, col_splits, ptr(ws), ws.numel(), ptr(out), stream_ptr())
    return out


def manifold_counts(queries: torch.Tensor, support: torch.Tensor, rad2: Optional[torch.Tensor], col_splits: int = 0, norms_q: Optional[torch.Tensor] = None,
                    norms_s: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(count, dmin2)`` per query row: ``count[q] = #{i : d2(q, s_i) <= rad2[i]}`` (int32) and ``dmin2[q] = min_i d2(q, s_i)`` (fp64, +inf if every distance is
    NaN), for (nq, D) and (ns, D) fp32 device tensors and the supports' (ns,) fp64 ``rad2`` (None: the counts are zero, only the minima are formed).  Two launches
    (one more per side without its norms), no host read; the same bits for every ``col_splits``."""
    nq, D, sq = _rows(queries, None, "manifold_counts: queries")
    ns, _, ss = _rows(support, D, "manifold_counts: support")
    col_splits = _splits(col_splits, "manifold_counts")
    if nq * ns >= 2 ** 53:
        raise NativeError(f"manifold_counts: nq * ns must stay below 2^53, got {nq} x {ns}")
    if rad2 is not None:
        _vector(rad2, ns, torch.float64, "manifold_counts: rad2")
    norms_q = row_norms(queries) if norms_q is None else _vector(norms_q, nq, torch.float64, "manifold_counts: norms_q")
    norms_s = row_norms(support) if norms_s is None else _vector(norms_s, ns, torch.float64, "manifold_counts: norms_s")
    need = int(lib().dcv_eval_manifold_workspace_bytes(nq, ns, col_splits))
    ws = N.scratch.get("eval_manifold", need, queries.device)
    count = torch.empty((nq,), dtype=torch.int32, device=queries.device)
    dmin2 = torch.empty((nq,), dtype=torch.float64, device=queries.device)
    _call("dcv_eval_manifold_counts", 2, ptr(queries), sq, nq, ptr(norms_q), ptr(support), ss, ns, ptr(norms_s), ptr(rad2), D, col_splits, ptr(ws), ws.numel(),
          ptr(count), ptr(dmin2), stream_ptr())
    return count, dmin2


def _metric_names(metrics, what: str) -> Tuple[str, ...]:
    metrics = tuple(metrics)
    if not metrics or any(m not in ("pr", "dc") for m in metrics):
        raise ValueError(f'{what}: metrics are chosen from ("pr", "dc"), got {metrics}')
    return metrics


def manifold_launches(k_pr: int = 3, k_dc: int = 5, metrics: Sequence[str] = ("pr", "dc")) -> int:
    """The launches of one ``manifold_metrics`` call: 2 for the norms, 2 per radius vector, 3 per counts call with its reduction — 17 at the defaults, 12 for "pr"
    alone or for both pairs with one k, 10 for "dc" alone."""
    pr, dc = "pr" in metrics, "dc" in metrics
    radii = (2 if pr else 0) + (1 if dc and not (pr and k_pr == k_dc) else 0)            # rA and rB at k_pr; rA at k_dc unless it is the same vector
    counts = 2 + (1 if pr and dc and k_pr != k_dc else 0)                                  # B against A, A against B; B against A again with the other radii
    return 2 + 2 * radii + 3 * counts


def manifold_metrics(real_feats: torch.Tensor, fake_feats: torch.Tensor, k_pr: int = 3, k_dc: int = 5, metrics: Sequence[str] = ("pr", "dc")) -> dict:
    """Improved precision and recall (Kynkäänniemi et al. 2019; "pr", k = 3) and density and coverage (Naeem et al. 2020; "dc", k = 5) between the rows of
    ``real_feats`` (na, D) and ``fake_feats`` (nb, D), fp32 device tensors -> ``{"precision", "recall", "density", "coverage"}`` (the requested pairs) as Python
    floats.  With rA, rB the squared k-th-neighbour radii of each side::

        precision = #{j : exists i, d2(b_j, a_i) <= rA[i]} / nb        recall   = #{i : exists j, d2(a_i, b_j) <= rB[j]} / na
        density   = sum_j #{i : d2(b_j, a_i) <= rA[i]} / (k nb)        coverage = #{i : min_j d2(a_i, b_j) <= rA[i]} / na

    Every comparison is ``<=`` (Kynkäänniemi's convention).  The ``prdc`` package uses ``<`` for density and coverage; the two differ on exact ties only.  If a row
    norm of either side is not finite, all requested metrics are NaN.  The norms are computed once per side, each radius vector once per distinct k, and the reduced
    integers come back in one small device-to-host read at the end (``manifold_launches`` launches)."""
    metrics = _metric_names(metrics, "manifold_metrics")
    na, D, _ = _rows(real_feats, None, "manifold_metrics: real features")
    nb, _, _ = _rows(fake_feats, D, "manifold_metrics: fake features")
    pr, dc = "pr" in metrics, "dc" in metrics
    k_pr, k_dc = _k(k_pr, "manifold_metrics: k_pr"), _k(k_dc, "manifold_metrics: k_dc")
    need = max(k_pr if pr else 0, k_dc if dc else 0) + 1
    if na < need or (pr and nb < k_pr + 1):
        raise NativeError(f"manifold_metrics: the k-th neighbour needs k + 1 rows (k_pr {k_pr}, k_dc {k_dc}), got {na} real and {nb} fake")
    if na * nb >= 2 ** 53:
        raise NativeError(f"manifold_metrics: na * nb must stay below 2^53, got {na} x {nb}")
    norm_a, norm_b = row_norms(real_feats), row_norms(fake_feats)
    out = torch.empty((3, 4), dtype=torch.float64, device=real_feats.device)      # one row per reduction

    def reduce(row, count, dmin2, own_rad2, norms, n):
        _call("dcv_eval_manifold_reduce", 1, ptr(count), ptr(dmin2), ptr(own_rad2), ptr(norms), n, ptr(out[row]), stream_ptr())

    radii_a = {}
    for k in ([k_pr] if pr else []) + ([k_dc] if dc else []):
        if k not in radii_a:
            radii_a[k] = knn_radii(real_feats, k, norms=norm_a)
    k_first = k_pr if pr else k_dc
    c, m = manifold_counts(fake_feats, real_feats, radii_a[k_first], norms_q=norm_b, norms_s=norm_a)      # precision, and density when it shares the radii
    reduce(0, c, m, None, norm_b, nb)
    rad_b = knn_radii(fake_feats, k_pr, norms=norm_b) if pr else None
    c, m = manifold_counts(real_feats, fake_feats, rad_b, norms_q=norm_a, norms_s=norm_b)                  # recall, and coverage's minima
    reduce(1, c, m, radii_a[k_dc] if dc else None, norm_a, na)
    if pr and dc and k_dc != k_pr:
        c, m = manifold_counts(fake_feats, real_feats, radii_a[k_dc], norms_q=norm_b, norms_s=norm_a)     # density
        reduce(2, c, m, None, norm_b, nb)
    o = out.cpu().numpy()
    dens = o[2] if (pr and dc and k_dc != k_pr) else o[0]
    bad = o[0, 3] + o[1, 3] > 0
    res = {}
    if pr:
        res["precision"], res["recall"] = float(o[0, 0] / nb), float(o[1, 0] / na)
    if dc:
        res["density"], res["coverage"] = float(dens[1] / (float(k_dc) * nb)), float(o[1, 2] / na)
    return {key: float("nan") for key in res} if bad else res


def _norms_host(x: np.ndarray) -> np.ndarray:
    s = np.zeros(x.shape[0], dtype=np.float64)
    for d in range(x.shape[1]):      # features ascending, as dcv_eval_row_norms adds them
        s = s + x[:, d] * x[:, d]
    return s


def d2_host(x, y) -> np.ndarray:
    """``d2(x_i, y_j) = max(0, (|x_i|^2 + |y_j|^2) - 2 x_i.y_j)`` in numpy fp64 for fp32 rows (a NaN stays a NaN)."""
    x, y = np.asarray(x, dtype=np.float32).astype(np.float64), np.asarray(y, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        t = (_norms_host(x)[:, None] + _norms_host(y)[None, :]) - 2.0 * (x @ y.T)
        return np.where(t < 0.0, 0.0, t)


def knn_radii_host(x, k: int) -> np.ndarray:
    """``rad2_k(X)``: per row the k-th smallest ``d2`` to the OTHER rows — self excluded by index, a NaN never selected, +inf where fewer than k survive."""
    k = _k(k, "knn_radii_host")
    d = d2_host(x, x)
    if d.shape[0] < k + 1:
        raise ValueError(f"knn_radii_host: the {k}-th neighbour needs at least {k + 1} rows, got {d.shape[0]}")
    np.fill_diagonal(d, np.inf)
    d[np.isnan(d)] = np.inf
    return np.sort(d, axis=1)[:, k - 1]


def counts_host(queries, support, rad2) -> Tuple[np.ndarray, np.ndarray]:
    """``(count, dmin2)`` of dcv_eval_manifold_counts: a NaN distance is in no ball and is no minimum; ``rad2`` None: zero counts."""
    d = d2_host(queries, support)
    with np.errstate(invalid="ignore"):
        count = np.zeros(d.shape[0], dtype=np.int32) if rad2 is None else (d <= np.asarray(rad2, dtype=np.float64)[None, :]).sum(axis=1).astype(np.int32)
    return count, np.where(np.isnan(d), np.inf, d).min(axis=1)


def manifold_host(a, b, k: int) -> dict:
    """The numpy fp64 mirror of the four metrics with one k — the specification the kernels are tested against, as ``draw_host`` is for the KID draw.  ->
    ``precision``, ``recall``, ``density``, ``coverage`` (floats; NaN, all four, if a row norm of either side is not finite) and what they are counted from:
    ``rad2_a``, ``rad2_b``, ``count_ba`` / ``dmin2_ba`` (fakes against reals and rA), ``count_ab`` / ``dmin2_ab`` (reals against fakes and rB)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1] or not 1 <= a.shape[1] <= MAX_DIM:
        raise ValueError(f"manifold_host: two (n, D) arrays with 1 <= D <= {MAX_DIM}, got {a.shape} and {b.shape}")
    ra, rb = knn_radii_host(a, k), knn_radii_host(b, k)
    c_ba, m_ba = counts_host(b, a, ra)
    c_ab, m_ab = counts_host(a, b, rb)
    na, nb = a.shape[0], b.shape[0]
    res = dict(precision=float((c_ba > 0).sum() / nb), recall=float((c_ab > 0).sum() / na), density=float(c_ba.astype(np.int64).sum() / (float(k) * nb)),
               coverage=float((m_ab <= ra).sum() / na))
    with np.errstate(all="ignore"):
        finite = np.isfinite(_norms_host(a.astype(np.float64))).all() and np.isfinite(_norms_host(b.astype(np.float64))).all()
    if not finite:
        res = {key: float("nan") for key in res}
    res.update(rad2_a=ra, rad2_b=rb, count_ba=c_ba, dmin2_ba=m_ba, count_ab=c_ab, dmin2_ab=m_ab)
    return res


# --------------------------------------------------------------------------- #
# PRD: k-means over the union of the two feature sets, and the precision-recall curve
# --------------------------------------------------------------------------- #
def _prd_int(v, lo: int, hi: int, name: str, what: str) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{what}: {lo} <= {name} <= {hi}, got {v!r}")
    return int(v)


def _prd_seed_value(seed, what: str) -> int:
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"{what}: the seed is an integer, got {seed!r}")
    return int(seed)


def _prd_sides(real, fake, what: str):
    na, D, sa = _rows(real, None, f"{what}: real features")
    nb, _, sb = _rows(fake, D, f"{what}: fake features")
    if na + nb >= 2 ** 31:
        raise NativeError(f"{what}: the union must have fewer than 2^31 rows, got {na} + {nb}")
    if fake.device != real.device:
        raise NativeError(f"{what}: the two sides are on {real.device} and {fake.device}")
    return na, nb, D, sa, sb


def _prd_table(t, shape, dtype, device, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != device or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        got = f"{t.dtype}{tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise NativeError(f"{what}: expected a contiguous {tuple(shape)} {dtype} tensor on {device}, got {got}")
    return t


def _prd_cent(cent, D: int, n: int, device, what: str) -> Tuple[int, int]:
    if not isinstance(cent, torch.Tensor) or cent.dim() != 3:
        got = tuple(cent.shape) if isinstance(cent, torch.Tensor) else type(cent).__name__
        raise NativeError(f"{what}: the centroids are a (R, C, {D}) float64 device tensor, got {got}")
    R, C = int(cent.shape[0]), int(cent.shape[1])
    if not 1 <= R <= PRD_MAX_RUNS or not 1 <= C <= PRD_MAX_CLUSTERS or C > n:
        raise NativeError(f"{what}: 1 <= R <= {PRD_MAX_RUNS} runs and 1 <= C <= min({PRD_MAX_CLUSTERS}, n = {n}) clusters, got centroids {tuple(cent.shape)}")
    _prd_table(cent, (R, C, D), torch.float64, device, f"{what}: centroids")
    return R, C


def _prd_norms(real, fake, norms_a, norms_b, na: int, nb: int, what: str):
    if norms_a is not None:      # what the caller hands over is checked before a missing side is launched
        _vector(norms_a, na, torch.float64, f"{what}: norms_a")
    if norms_b is not None:
        _vector(norms_b, nb, torch.float64, f"{what}: norms_b")
    return row_norms(real) if norms_a is None else norms_a, row_norms(fake) if norms_b is None else norms_b


def _keyed_perm_host(x: np.ndarray, n_rows: int, e0, e1, k0: int, k1: int) -> np.ndarray:
    """perm(x) on [0, n_rows) for uint64 arrays x, e0 (and a scalar e1): the bijection ``draw_host`` walks, the counter's last two words given."""
    h = clipstore.half_bits(n_rows)
    mask = np.uint64((1 << h) - 1)
    x = np.array(x, dtype=np.uint64)
    e0 = np.broadcast_to(np.asarray(e0, dtype=np.uint64), x.shape)
    todo = np.ones(x.shape, dtype=bool)
    while todo.any():      # cycle walking: only the values still outside [0, n_rows) go round again
        v = x[todo]
        L, R = v >> np.uint64(h), v & mask
        for r in range(clipstore.FEISTEL_ROUNDS):
            f = clipstore.philox4x32_10(R, r, e0[todo], e1, k0, k1)[0] & mask
            L, R = R, L ^ f
        v = (L << np.uint64(h)) | R
        x[todo] = v
        todo[todo] = v >= np.uint64(n_rows)
    return x


def prd_seed_host(seed: int, num_runs: int, num_clusters: int, n: int) -> np.ndarray:
    """The (R, C) int32 union rows dcv_eval_prd_seed starts the centroids from — integers only, the specification of the kernel.  rows[r][c] = perm_r(c): the clip
    store's keyed bijection on [0, n) (what ``draw_host`` uses) with key = seed + PRD_SALT and the Philox counter {R, round, r, 0}; a run's rows are distinct."""
    R, C, n = int(num_runs), int(num_clusters), int(n)
    if not (1 <= R <= PRD_MAX_RUNS and 1 <= C <= PRD_MAX_CLUSTERS and C <= n < 2 ** 31):
        raise ValueError(f"prd_seed_host: 1 <= R <= {PRD_MAX_RUNS}, 1 <= C <= {PRD_MAX_CLUSTERS}, C <= n < 2^31; got {R}, {C}, {n}")
    key = (int(seed) + PRD_SALT) & _M64
    x = np.tile(np.arange(C, dtype=np.uint64), R)
    runs = np.repeat(np.arange(R, dtype=np.uint64), C)
    return _keyed_perm_host(x, n, runs, 0, key & 0xFFFFFFFF, key >> 32).reshape(R, C).astype(np.int32)


def prd_seed(real: torch.Tensor, fake: torch.Tensor, num_clusters: int = 20, num_runs: int = 10, seed: int = 0) -> torch.Tensor:
    """The (R, C, D) fp64 device tensor of starting centroids: union row ``prd_seed_host(seed, R, C, n)[r][c]`` as doubles.  One launch."""
    na, nb, D, sa, sb = _prd_sides(real, fake, "prd_seed")
    C, R = _prd_int(num_clusters, 1, PRD_MAX_CLUSTERS, "num_clusters", "prd_seed"), _prd_int(num_runs, 1, PRD_MAX_RUNS, "num_runs", "prd_seed")
    seed = _prd_seed_value(seed, "prd_seed")
    if C > na + nb:
        raise NativeError(f"prd_seed: {C} clusters need at least as many rows, got {na} + {nb}")
    cent = torch.empty((R, C, D), dtype=torch.float64, device=real.device)
    _call("dcv_eval_prd_seed", 1, ptr(real), sa, na, ptr(fake), sb, nb, D, C, R, seed & _M64, ptr(cent), stream_ptr())
    return cent


def prd_assign(real: torch.Tensor, fake: torch.Tensor, cent: torch.Tensor, norms_a: Optional[torch.Tensor] = None,
               norms_b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The (R, n) int32 device tensor ``assign[r][u]``: the LOWEST cluster c of minimal ``cn[r][c] - 2 x_u . cent[r][c]`` among the scores that are not NaN, for
    union row u (the ``real`` rows, then the ``fake`` rows); C, "unassigned", for a row whose norm is not finite or that has no comparable score.  ``norms_a`` /
    ``norms_b``: ``row_norms`` of the sides if the caller has them.  Two launches (one more per side without its norms), no host read."""
    na, nb, D, sa, sb = _prd_sides(real, fake, "prd_assign")
    R, C = _prd_cent(cent, D, na + nb, real.device, "prd_assign")
    norms_a, norms_b = _prd_norms(real, fake, norms_a, norms_b, na, nb, "prd_assign")
    need = int(lib().dcv_eval_prd_assign_workspace_bytes(C, R))
    ws = N.scratch.get("eval_prd_assign", need, real.device)
    assign = torch.empty((R, na + nb), dtype=torch.int32, device=real.device)
    _call("dcv_eval_prd_assign", 2, ptr(real), sa, na, ptr(fake), sb, nb, ptr(norms_a), ptr(norms_b), D, ptr(cent), C, R, ptr(assign), ptr(ws), ws.numel(),
          stream_ptr())
    return assign


def prd_count(assign: torch.Tensor, norms_a: torch.Tensor, norms_b: torch.Tensor, num_clusters: int) -> torch.Tensor:
    """The (R, 2, C + 1) int32 device tensor ``hist[r][side][c]``: the side's rows (0 = real) assigned to c; column C: the unassigned rows.  One launch."""
    C = _prd_int(num_clusters, 1, PRD_MAX_CLUSTERS, "num_clusters", "prd_count")
    if not isinstance(norms_a, torch.Tensor) or not isinstance(norms_b, torch.Tensor) or norms_a.dim() != 1 or norms_b.dim() != 1:
        raise NativeError("prd_count: the norms of the two sides are (na,) and (nb,) float64 device tensors")
    na, nb = int(norms_a.shape[0]), int(norms_b.shape[0])
    _vector(norms_a, na, torch.float64, "prd_count: norms_a")
    _vector(norms_b, nb, torch.float64, "prd_count: norms_b")
    if not isinstance(assign, torch.Tensor) or assign.dim() != 2 or not 1 <= assign.shape[0] <= PRD_MAX_RUNS or na < 1 or nb < 1:
        raise NativeError(f"prd_count: the assignments are a (R <= {PRD_MAX_RUNS}, na + nb) int32 device tensor")
    R = int(assign.shape[0])
    _prd_table(assign, (R, na + nb), torch.int32, norms_a.device, "prd_count: assignments")
    hist = torch.empty((R, 2, C + 1), dtype=torch.int32, device=assign.device)
    _call("dcv_eval_prd_count", 1, ptr(assign), ptr(norms_a), na, ptr(norms_b), nb, C, R, ptr(hist), stream_ptr())
    return hist


def prd_update(real: torch.Tensor, fake: torch.Tensor, assign: torch.Tensor, cent: torch.Tensor, row_splits: int = 0, norms_a: Optional[torch.Tensor] = None,
               norms_b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One Lloyd update, ``cent`` in place: ``cent[r][c] = (sum of the rows with assign[r][u] == c) / count`` in fp64 where the count is positive; an empty cluster
    keeps its centroid bit for bit (sklearn relocates it).  -> the (R, 2, C + 1) int32 device tensor ``hist`` of these assignments.  A row whose norm is not finite
    is left out and counted as unassigned whatever its entry.  ``row_splits``: the slabs the rows are summed in (0: the library chooses from the shapes alone); with
    integer features the result is the same bits for every value.  Three launches (one more per side without its norms), no host read."""
    na, nb, D, sa, sb = _prd_sides(real, fake, "prd_update")
    R, C = _prd_cent(cent, D, na + nb, real.device, "prd_update")
    _prd_table(assign, (R, na + nb), torch.int32, real.device, "prd_update: assignments")
    S = _prd_int(row_splits, 0, PRD_MAX_ROW_SPLITS, "row_splits", "prd_update")
    norms_a, norms_b = _prd_norms(real, fake, norms_a, norms_b, na, nb, "prd_update")
    need = int(lib().dcv_eval_prd_update_workspace_bytes(na + nb, D, C, R, S))
    ws = N.scratch.get("eval_prd_update", need, real.device)
    hist = torch.empty((R, 2, C + 1), dtype=torch.int32, device=real.device)
    _call("dcv_eval_prd_update", 3, ptr(real), sa, na, ptr(fake), sb, nb, ptr(norms_a), ptr(norms_b), ptr(assign), D, C, R, S, ptr(cent), ptr(hist), ptr(ws),
          ws.numel(), stream_ptr())
    return hist


def prd_launches(iters: int = 20, with_norms: bool = True) -> int:
    """The launches of one ``prd_kmeans`` / ``prd_metrics`` call: the two sides' norms (``with_norms``), 1 for the seeding, 2 + 3 per Lloyd iteration (assignment:
    cn and the sweep; update: counts, slab sums, fold), then the final assignment's 2 and its count's 1 — 106 at the default 20 iterations."""
    return (2 if with_norms else 0) + 1 + 5 * int(iters) + 3


def prd_kmeans(real: torch.Tensor, fake: torch.Tensor, num_clusters: int = 20, num_runs: int = 10, iters: int = 20, seed: int = 0,
               row_splits: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(hist, cent)`` on the device: ``num_runs`` independent k-means runs of ``num_clusters`` clusters over the union of the ``real`` (na, D) and ``fake`` (nb, D)
    fp32 device rows.  Seeding (``prd_seed``), then ``iters`` times assignment and update, then a final assignment and count: ``hist`` (R, 2, C + 1) int32 belongs to
    the final centroids ``cent`` (R, C, D) fp64.  Every iteration is launched (a converged one is a fixed point and changes no bit) and nothing is read back in
    between: ``prd_launches(iters)`` launches.  Full-batch Lloyd with a fixed number of iterations is this project's choice; the published PRD code runs mini-batch
    k-means, whose random batches have no fixed order of sums, and sklearn relocates an empty cluster where this one keeps its centroid."""
    na, nb, D, _, _ = _prd_sides(real, fake, "prd_kmeans")
    C, R = _prd_int(num_clusters, 1, PRD_MAX_CLUSTERS, "num_clusters", "prd_kmeans"), _prd_int(num_runs, 1, PRD_MAX_RUNS, "num_runs", "prd_kmeans")
    T, S = _prd_int(iters, 0, PRD_MAX_ITERS, "iters", "prd_kmeans"), _prd_int(row_splits, 0, PRD_MAX_ROW_SPLITS, "row_splits", "prd_kmeans")
    seed = _prd_seed_value(seed, "prd_kmeans")
    if C > na + nb:
        raise NativeError(f"prd_kmeans: {C} clusters need at least as many rows, got {na} + {nb}")
    norms_a, norms_b = row_norms(real), row_norms(fake)
    cent = prd_seed(real, fake, C, R, seed)
    for _ in range(T):
        assign = prd_assign(real, fake, cent, norms_a, norms_b)
        prd_update(real, fake, assign, cent, S, norms_a, norms_b)
    assign = prd_assign(real, fake, cent, norms_a, norms_b)
    return prd_count(assign, norms_a, norms_b, C), cent


def prd_curve(hist, num_angles: int = 1001) -> Tuple[np.ndarray, np.ndarray]:
    """``(precision, recall)``, two (num_angles,) fp64 arrays: the PRD curve of Sajjadi et al. 2018 from the (R, 2, C + 1) histograms (side 0 = real; column C: the
    unassigned rows), averaged over the runs.  Per run ``pr = hist[r][0][:C] / sum``, ``pf = hist[r][1][:C] / sum`` (each side normalised on its own: unequal sizes are
    fine), ``slope = tan(linspace(1e-10, pi / 2 - 1e-10, num_angles))``, ``precision[l] = sum_c min(pr_c slope_l, pf_c)``, ``recall[l] = precision[l] / slope_l``,
    both clipped to [0, 1].  If any run has an unassigned row, both curves are NaN.  The constants are the published code's as recalled — that code is not at hand, so
    this function is the specification."""
    h = np.asarray(hist)
    if h.ndim != 3 or h.shape[1] != 2 or h.shape[2] < 2 or h.shape[0] < 1 or not np.issubdtype(h.dtype, np.integer) or (h < 0).any():
        raise ValueError(f"prd_curve: a (R, 2, C + 1) table of counts, got {h.dtype}{h.shape}")
    num_angles = _prd_int(num_angles, 2, 1 << 20, "num_angles", "prd_curve")
    if h[:, :, -1].any():
        nan = np.full(num_angles, np.nan)
        return nan, nan.copy()
    h = h[:, :, :-1].astype(np.float64)
    if (h.sum(axis=2) == 0).any():
        raise ValueError("prd_curve: a side has no rows")
    slope = np.tan(np.linspace(1e-10, np.pi / 2 - 1e-10, num_angles))
    precision, recall = np.zeros(num_angles), np.zeros(num_angles)
    for r in range(h.shape[0]):
        pr, pf = h[r, 0] / h[r, 0].sum(), h[r, 1] / h[r, 1].sum()
        p = np.minimum(pr[None, :] * slope[:, None], pf[None, :]).sum(axis=1)
        precision += np.clip(p, 0.0, 1.0)
        recall += np.clip(p / slope, 0.0, 1.0)
    return precision / h.shape[0], recall / h.shape[0]


def prd_f_beta(precision, recall, beta: float = 8) -> float:
    """``max_l (1 + beta^2) p_l r_l / (beta^2 p_l + r_l + 1e-10)`` over the curve: beta = 8 weighs recall, beta = 1 / 8 precision.  NaN for a NaN curve."""
    p, r = np.asarray(precision, dtype=np.float64), np.asarray(recall, dtype=np.float64)
    if p.shape != r.shape or p.ndim != 1 or p.size < 1 or not float(beta) > 0.0:
        raise ValueError(f"prd_f_beta: two curves of one length and beta > 0, got {p.shape}, {r.shape}, {beta!r}")
    if np.isnan(p).any() or np.isnan(r).any():
        return float("nan")
    b2 = float(beta) ** 2
    return float(np.max((1.0 + b2) * p * r / (b2 * p + r + 1e-10)))


def _prd_scores(hist, num_angles: int = 1001) -> dict:
    p, r = prd_curve(hist, num_angles)
    return {"prd_f8": prd_f_beta(p, r, 8), "prd_f1_8": prd_f_beta(p, r, 1.0 / 8.0)}


def prd_metrics(real: torch.Tensor, fake: torch.Tensor, num_clusters: int = 20, num_runs: int = 10, iters: int = 20, seed: int = 0, row_splits: int = 0) -> dict:
    """``{"prd_f8", "prd_f1_8"}`` as Python floats: ``prd_kmeans`` on the device, ONE device-to-host read of its histograms (R x 2 x (C + 1) integers), then
    ``prd_curve`` and ``prd_f_beta`` in host fp64.  ``prd_f8`` is F_8 (recall-weighted), ``prd_f1_8`` F_1/8 (precision-weighted); both NaN if a feature is not
    finite.  The cluster and run counts follow the published PRD code; see ``prd_kmeans`` for what differs from it."""
    hist, _ = prd_kmeans(real, fake, num_clusters, num_runs, iters, seed, row_splits)
    return _prd_scores(hist.cpu().numpy())


def _prd_assign_host(x: np.ndarray, norms: np.ndarray, cent: np.ndarray) -> np.ndarray:
    """(R, n) int32: the mirror of dcv_eval_prd_assign for fp64 rows x (n, D), their norms and centroids (R, C, D)."""
    R, C, D = cent.shape
    out = np.empty((R, x.shape[0]), dtype=np.int32)
    with np.errstate(all="ignore"):
        ok = np.isfinite(norms)
        for r in range(R):
            cn = _norms_host(cent[r])
            score = cn[None, :] - 2.0 * (x @ cent[r].T)
            valid = ~np.isnan(score)
            masked = np.where(valid, score, np.inf)
            first = (valid & (masked == masked.min(axis=1, keepdims=True))).argmax(axis=1)      # the lowest index of the minimum among the comparable ones
            out[r] = np.where(ok & valid.any(axis=1), first, C)
    return out


def _prd_count_host(assign: np.ndarray, norms: np.ndarray, na: int, C: int) -> np.ndarray:
    R, n = assign.shape
    hist = np.zeros((R, 2, C + 1), dtype=np.int32)
    ok = np.isfinite(norms)
    for r in range(R):
        slot = np.where(ok & (assign[r] >= 0) & (assign[r] < C), assign[r], C)
        hist[r, 0] = np.bincount(slot[:na], minlength=C + 1)
        hist[r, 1] = np.bincount(slot[na:], minlength=C + 1)
    return hist


def _prd_update_host(x: np.ndarray, norms: np.ndarray, na: int, assign: np.ndarray, cent: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(cent', hist): the mirror of dcv_eval_prd_update; the rows of a cluster are added in ascending order."""
    R, C, D = cent.shape
    hist = _prd_count_host(assign, norms, na, C)
    new = cent.copy()
    ok = np.isfinite(norms)
    for r in range(R):
        for c in range(C):
            rows = np.flatnonzero(ok & (assign[r] == c))
            if rows.size:
                new[r, c] = np.add.accumulate(x[rows], axis=0)[-1] / float(rows.size)      # accumulate: strictly one row after the other
    return new, hist


def prd_host(real, fake, num_clusters: int = 20, num_runs: int = 10, iters: int = 20, seed: int = 0, cent=None) -> dict:
    """The numpy fp64 mirror of ``prd_metrics`` — the specification the kernels are tested against.  -> ``assign``: the T + 1 assignments (R, n) int32, ``cent``: the
    T + 1 centroid tensors (R, C, D) (``cent[t]`` is what ``assign[t]`` was formed against: ``cent[0]`` the seeds), ``hist``: the T + 1 histograms (R, 2, C + 1),
    ``seed_rows`` (R, C), and ``prd_f8`` / ``prd_f1_8`` of the last histogram.  ``cent``: explicit starting centroids instead of the seeding."""
    a, b = np.asarray(real, dtype=np.float32), np.asarray(fake, dtype=np.float32)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1] or not 1 <= a.shape[1] <= MAX_DIM or a.shape[0] < 1 or b.shape[0] < 1:
        raise ValueError(f"prd_host: two (n, D) arrays with 1 <= D <= {MAX_DIM}, got {a.shape} and {b.shape}")
    C, R = _prd_int(num_clusters, 1, PRD_MAX_CLUSTERS, "num_clusters", "prd_host"), _prd_int(num_runs, 1, PRD_MAX_RUNS, "num_runs", "prd_host")
    T = _prd_int(iters, 0, PRD_MAX_ITERS, "iters", "prd_host")
    na, n = a.shape[0], a.shape[0] + b.shape[0]
    if C > n:
        raise ValueError(f"prd_host: {C} clusters need at least as many rows, got {n}")
    x = np.concatenate([a, b]).astype(np.float64)
    with np.errstate(all="ignore"):
        norms = _norms_host(x)
    rows = prd_seed_host(seed, R, C, n)
    c = x[rows] if cent is None else np.array(cent, dtype=np.float64).reshape(R, C, a.shape[1])
    assigns, cents, hists = [], [], []
    for t in range(T + 1):
        with np.errstate(all="ignore"):
            assign = _prd_assign_host(x, norms, c)
            cents.append(c)
            assigns.append(assign)
            if t < T:
                c, hist = _prd_update_host(x, norms, na, assign, c)
            else:
                hist = _prd_count_host(assign, norms, na, C)
            hists.append(hist)
    out = dict(assign=assigns, cent=cents, hist=hists, seed_rows=rows)
    out.update(_prd_scores(hists[-1]))
    return out


# --------------------------------------------------------------------------- #
# generator -> extractor -> statistics
# --------------------------------------------------------------------------- #
class Evaluator:
    """``Evaluator(extractor, metrics=("is", "fid", "kid"), max_features=50000)``: the replacement of ``Trainer.evaluate`` (trainer.py:171-224).  ``metrics`` are chosen
    from ``("is", "fid", "kid", "pr", "dc", "prcurve")``: "pr" adds improved precision and recall (``pr_k`` = 3 neighbours), "dc" density and coverage (``dc_k`` = 5),
    both over the stored features of the two sides (``manifold_metrics``).  "prcurve" is the reference's ``"prd"`` (trainer.py:216-219; the name "prd" itself stays
    refused): ``prd_metrics`` over the stored features with ``prd_clusters`` = 20, ``prd_runs`` = 10, ``prd_iters`` = 20 and the Evaluator's seed, adding
    ``"prd_f8"`` and ``"prd_f1_8"``.  Like "pr" and "dc" it is not additive across data-parallel ranks: gathering the features is the caller's.

    ``extractor(xc)`` takes a (B, 3, T, H, W) fp32 device clip in [-1, 1] and returns ``(features (B, D), logits (B, K) or None)`` on the device — the caller's
    network (the reference's is a Kinetics ResNeXt-101).  ``observe_real(xc)`` feeds real batches (a ``clipstore.ClipSampler``'s ``batch["color"]`` for instance);
    the real statistics are computed once, ``real.save(path)`` keeps them and ``real_moments=FeatureMoments.load(path)`` brings them back (enough for "fid"; "kid",
    "pr" and "dc" need real features).  ``evaluate(ggen, cgen, num_samples, batchsize)`` samples as ``sampling.generate_samples`` does and returns Python floats.

    Features for the kernel distance and the manifold metrics go to device buffers of at most ``max_features`` rows per side, allocated once (on the first batch, when D is known) and
    filled by the library's strided copy; rows past the buffer still enter the moments."""

    def __init__(self, extractor: Callable, metrics: Sequence[str] = DEFAULT_METRICS, max_features: int = 50000, kid_subsets: int = 100, kid_subset_size: int = 1000,
                 seed: int = 0, real_moments: Optional[FeatureMoments] = None, prd_clusters: int = 20, prd_runs: int = 10, prd_iters: int = 20, pr_k: int = 3,
                 dc_k: int = 5):
        metrics = tuple(metrics)
        unknown = [m for m in metrics if m not in METRICS]
        if unknown or not metrics:
            raise ValueError(f"Evaluator: metrics are chosen from {METRICS}, got {metrics}")
        if not callable(extractor):
            raise TypeError("Evaluator: the extractor must be callable")
        if int(max_features) < 2:
            raise ValueError(f"Evaluator: max_features >= 2, got {max_features}")
        self.extractor, self.metrics, self.max_features = extractor, metrics, int(max_features)
        self.kid_subsets, self.kid_subset_size, self.seed = int(kid_subsets), int(kid_subset_size), int(seed)
        self.pr_k, self.dc_k = _k(pr_k, "Evaluator: pr_k"), _k(dc_k, "Evaluator: dc_k")
        self.prd_clusters = _prd_int(prd_clusters, 1, PRD_MAX_CLUSTERS, "prd_clusters", "Evaluator")
        self.prd_runs, self.prd_iters = _prd_int(prd_runs, 1, PRD_MAX_RUNS, "prd_runs", "Evaluator"), _prd_int(prd_iters, 0, PRD_MAX_ITERS, "prd_iters", "Evaluator")
        self._stores = any(m in metrics for m in ("kid", "pr", "dc", "prcurve"))      # the metrics computed from the stored features of both sides
        self.real: Optional[FeatureMoments] = real_moments
        self.real_feats: Optional[torch.Tensor] = None      # (max_features, D) fp32, the first n_real_feats rows filled
        self.n_real_feats = 0
        self.fake: Optional[FeatureMoments] = None           # of the last evaluate()
        self.inception: Optional[InceptionStats] = None
        self.fake_feats: Optional[torch.Tensor] = None
        self.n_fake_feats = 0
        self.ggen = self.cgen = None      # the generators evaluate() samples when it is given none (trainer.build_evaluator binds them)

    @staticmethod
    def _clip(xc, what: str):
        if not isinstance(xc, torch.Tensor):
            raise NativeError(f"{what}: expected a tensor, got {type(xc).__name__}")
        N._require(xc, what)
        if xc.dim() != 5:
            raise NativeError(f"{what}: expected a (B, C, T, H, W) clip, got {tuple(xc.shape)}")

    def _extract(self, xc, what: str):
        out = self.extractor(xc)
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise NativeError(f"{what}: the extractor must return (features, logits or None)")
        feats, logits = out
        _rows(feats, None, f"{what}: features")
        if feats.shape[0] != xc.shape[0]:
            raise NativeError(f"{what}: {xc.shape[0]} clips in, {feats.shape[0]} feature rows out")
        if logits is not None:
            _rows(logits, None, f"{what}: logits")
            if logits.shape[0] != xc.shape[0]:
                raise NativeError(f"{what}: {xc.shape[0]} clips in, {logits.shape[0]} logit rows out")
        return feats, logits

    def _store(self, buf: Optional[torch.Tensor], filled: int, feats: torch.Tensor):
        """Append feats' rows to the side's buffer with dcv_axpby (one launch), as far as it has room."""
        from . import ops
        if buf is None:
            buf = torch.empty((self.max_features, feats.shape[1]), dtype=torch.float32, device=feats.device)
        if buf.shape[1] != feats.shape[1]:
            raise NativeError(f"Evaluator: the extractor's features have {feats.shape[1]} values, the stored ones {buf.shape[1]}")
        k = min(int(feats.shape[0]), self.max_features - filled)
        if k > 0:
            ops._axpby(feats[:k], 1.0, None, 0.0, buf[filled:filled + k])
            _STATS["launches"] += 1
        return buf, filled + max(k, 0)

    def observe_real(self, xc: torch.Tensor) -> None:
        """One real batch: its features enter the real moments and, for the kernel distance and the manifold metrics, the real feature buffer.  The logits are not
        used."""
        self._clip(xc, "Evaluator.observe_real")
        with torch.no_grad():
            feats, _ = self._extract(xc, "Evaluator.observe_real")
            if "fid" in self.metrics:      # the Gram is accumulated only where the Fréchet distance is asked for
                if self.real is None:
                    self.real = FeatureMoments(feats.shape[1], feats.device)
                self.real.update(feats)
            if self._stores:
                self.real_feats, self.n_real_feats = self._store(self.real_feats, self.n_real_feats, feats)

    def _refuse_missing(self, num_samples: int):
        if "fid" in self.metrics and (self.real is None or self.real.n < 2):
            raise NativeError('Evaluator: "fid" needs the real statistics (observe_real() on at least two clips, or real_moments=FeatureMoments.load(...))')
        if "kid" in self.metrics and self.n_real_feats < 2:
            raise NativeError('Evaluator: "kid" needs real features (observe_real() on at least two clips)')
        for name, k in (("pr", self.pr_k), ("dc", self.dc_k)):      # the k-th neighbour of a row is among the OTHER rows of its side
            if name in self.metrics and self.n_real_feats < k + 1:
                raise NativeError(f'Evaluator: "{name}" with k = {k} needs at least {k + 1} real features (observe_real() saw {self.n_real_feats})')
            if name in self.metrics and min(num_samples, self.max_features) < k + 1:
                raise NativeError(f'Evaluator: "{name}" with k = {k} needs at least {k + 1} generated samples within max_features, got num_samples {num_samples}, '
                                  f'max_features {self.max_features}')
        if "prcurve" in self.metrics:
            if self.n_real_feats < 1:
                raise NativeError('Evaluator: "prcurve" needs real features (observe_real() on at least one clip)')
            if self.n_real_feats + min(num_samples, self.max_features) < self.prd_clusters:
                raise NativeError(f'Evaluator: "prcurve" with {self.prd_clusters} clusters needs at least as many rows, got {self.n_real_feats} real features and '
                                  f'num_samples {num_samples} within max_features {self.max_features}')

    def evaluate(self, ggen=None, cgen=None, num_samples: int = 0, batchsize: int = 20) -> dict:
        """Generate ``num_samples`` clips in batches of ``batchsize`` (eval mode, no_grad, the last batch truncated), run the extractor on each batch and accumulate;
        then finalise.  -> ``{"is": .., "fid": .., "kid": .., "kid_std": .., "precision": .., "recall": .., "density": .., "coverage": .., "prd_f8": .., "prd_f1_8": ..}`` (the requested ones) as
        Python floats.  A metric whose inputs are missing is refused
        by name before this module launches anything.  ``ggen`` / ``cgen`` default to the generators trainer.build_evaluator bound."""
        ggen, cgen = ggen if ggen is not None else self.ggen, cgen if cgen is not None else self.cgen
        if ggen is None or cgen is None:
            raise ValueError("Evaluator.evaluate: no generators (pass ggen and cgen, or build the evaluator with trainer.build_evaluator)")
        num_samples, batchsize = int(num_samples), int(batchsize)
        if num_samples < 2 or batchsize < 1:
            raise ValueError(f"Evaluator.evaluate: num_samples >= 2 and batchsize >= 1, got {num_samples}, {batchsize}")
        self._refuse_missing(num_samples)
        ggen.eval()
        cgen.eval()
        self.n_fake_feats = 0
        first = True
        for start in range(0, num_samples, batchsize):
            k = min(batchsize, num_samples - start)
            with torch.no_grad():
                xg = ggen.sample_videos(batchsize)
                xc = cgen.forward_videos(xg)
                self._clip(xc, "Evaluator.evaluate: the colour generator's output")
                feats, logits = self._extract(xc, "Evaluator.evaluate")
                if "is" in self.metrics and logits is None:
                    raise NativeError('Evaluator: "is" needs logits, and the extractor returned None for them')
                if first:      # the states of the last evaluate() are cleared in place and used again; one is made only for a metric that was asked for
                    first = False
                    if "fid" in self.metrics:
                        if self.real.dim != feats.shape[1]:
                            raise NativeError(f"Evaluator: the real statistics have {self.real.dim} features, the extractor returns {feats.shape[1]}")
                        if self.fake is not None and self.fake.dim == feats.shape[1] and self.fake.device == feats.device:
                            self.fake.reset()
                        else:
                            self.fake = FeatureMoments(feats.shape[1], feats.device)
                    if "is" in self.metrics:
                        if self.inception is not None and self.inception.num_classes == logits.shape[1] and self.inception.device == logits.device:
                            self.inception.reset()
                        else:
                            self.inception = InceptionStats(logits.shape[1], logits.device)
                feats = feats[:k]
                if "fid" in self.metrics:
                    self.fake.update(feats)
                if "is" in self.metrics:
                    self.inception.update(logits[:k])
                if self._stores:
                    self.fake_feats, self.n_fake_feats = self._store(self.fake_feats, self.n_fake_feats, feats)
        out = {}
        if "is" in self.metrics:
            out["is"] = self.inception.score()
        if "fid" in self.metrics:
            out["fid"] = frechet_distance(self.real, self.fake)
        if "kid" in self.metrics:
            out["kid"], out["kid_std"] = kernel_distance(self.real_feats[:self.n_real_feats], self.fake_feats[:self.n_fake_feats], self.kid_subsets,
                                                         self.kid_subset_size, self.seed)
        wanted = tuple(m for m in ("pr", "dc") if m in self.metrics)
        if wanted:
            out.update(manifold_metrics(self.real_feats[:self.n_real_feats], self.fake_feats[:self.n_fake_feats], self.pr_k, self.dc_k, wanted))
        if "prcurve" in self.metrics:
            out.update(prd_metrics(self.real_feats[:self.n_real_feats], self.fake_feats[:self.n_fake_feats], self.prd_clusters, self.prd_runs, self.prd_iters, self.seed))
        return out
