"""Host reference, in numpy, of the inverse neighbour lists and of every kernel that sums over them in list order
(nsdp_segment_sum_rows*, nsdp_scatter_cm_lists, nsdp_three_interpolate_grad_lists), written from the contract in
include/nsdp_hip.h and include/nsdp_scatter.h, not from the kernels:

  * ``inverse_lists_ref``: the lists are the stable sort of the entry numbers by source index; the offsets the exclusive scan
    of the counts;
  * ``list_sums``: every list is added to +0 term by term, in list order, one fp32 rounding per addition -- what a kernel that
    keeps the contract returns bit for bit (none of them multiplies inside the sum except the interpolation form, whose product
    is rounded on its own: csrc/pointnet2_ops.hip is built without contraction);
  * ``sliced_list_sums``: the order of the sliced kernels for a list longer than they take as ascending;
  * ``exact_sums`` / ``bound``: the fp64 sum of the same fp32 terms and the forward bound of a recursive fp32 sum, for the
    comparisons that cannot be exact;
  * ``make_idx`` / ``make_terms`` / ``reversed_lists`` / ``order_matters``: the generator of the GPU tests and the check that an
    exact comparison on its data is not vacuous (the same lists summed backwards give other bits).

One shape per call: offsets [N + 1], entries [E]; the tests loop over the shapes of a batch."""
import numpy as np

F = np.float32
U = 2.0 ** -24


def inverse_lists_ref(idx, N):
    """idx [B, ...] integers in [0, N) -> (offsets [B, N + 1] int32, entries [B, E] int32)."""
    flat = np.asarray(idx).reshape(np.asarray(idx).shape[0], -1).astype(np.int64)
    assert flat.size == 0 or (flat.min() >= 0 and flat.max() < N)
    entries = np.argsort(flat, axis=1, kind="stable").astype(np.int32)
    offsets = np.zeros((flat.shape[0], N + 1), dtype=np.int64)
    for b in range(flat.shape[0]):
        offsets[b, 1:] = np.cumsum(np.bincount(flat[b], minlength=N))
    return offsets.astype(np.int32), entries


def _term_rows(terms, e, weights):
    """The fp32 terms of the entries e: terms[e], or fl32(terms[e // 3] * weights[e]) in the interpolation form."""
    if weights is None:
        return terms[e]
    return terms[e // 3] * weights[e][:, None]


def _checked(terms, offsets, entries, weights):
    terms = np.ascontiguousarray(terms)
    assert terms.dtype == F and terms.ndim == 2
    offsets, entries = np.asarray(offsets).astype(np.int64), np.asarray(entries).astype(np.int64)
    assert offsets.ndim == 1 and entries.ndim == 1 and offsets[0] == 0 and offsets[-1] == entries.size
    if weights is None:
        assert terms.shape[0] == entries.size
    else:
        weights = np.ascontiguousarray(weights)
        assert weights.dtype == F and weights.shape == (entries.size,) and entries.size == 3 * terms.shape[0]
    return terms, offsets, entries, weights


def list_sums(terms, offsets, entries, weights=None):
    """terms [E, d] fp32 (or [n, d] with weights [3 n]) -> [N, d] fp32: every list added to +0 in list order.  Step j adds the
    j-th entry of every list that has one, so the Python loop is as long as the longest list."""
    terms, offsets, entries, weights = _checked(terms, offsets, entries, weights)
    lengths = np.diff(offsets)
    order = np.argsort(-lengths, kind="stable")                  # sources, the longest list first
    alive = np.searchsorted(-lengths[order], -np.arange(int(lengths.max(initial=0))), side="left")
    acc = np.zeros((lengths.size, terms.shape[1]), dtype=F)
    for j, count in enumerate(alive):                            # count = lists with more than j entries
        live = order[:count]
        acc[live] = acc[live] + _term_rows(terms, entries[offsets[live] + j], weights)
    assert acc.dtype == F
    return acc


def sliced_list_sums(terms, offsets, entries, weights=None, *, slice, sort_max=1024):
    """The rule of scatter_cm_lists_sliced_kernel.  ``slice``: entry numbers per slice (three per staged row element in the
    interpolation form).  A list of up to ``sort_max`` entries is summed in list order.  A longer one is taken as unordered: the
    slices [0, slice), [slice, 2 slice), ... come in ascending order, and inside a slice the list is walked in its stored order
    and the entries that fall into the slice are added -- the list stably sorted by slice number.  For an ascending list that
    is list order."""
    _, off, ent, _ = _checked(terms, offsets, entries, weights)
    ent = ent.copy()
    for s in np.nonzero(np.diff(off) > sort_max)[0]:
        part = ent[off[s]:off[s + 1]]
        ent[off[s]:off[s + 1]] = part[np.argsort(part // slice, kind="stable")]
    return list_sums(terms, offsets, ent, weights)


def _per_list_f64(terms, offsets, entries, weights, absolute):
    terms, offsets, entries, weights = _checked(terms, offsets, entries, weights)
    rows = _term_rows(terms, entries, weights).astype(np.float64)      # (the product is rounded to fp32 first: the kernel's term)
    out = np.zeros((offsets.size - 1, terms.shape[1]), dtype=np.float64)
    np.add.at(out, np.repeat(np.arange(offsets.size - 1), np.diff(offsets)), np.abs(rows) if absolute else rows)
    return out


def exact_sums(terms, offsets, entries, weights=None):
    """[N, d] fp64: the sum of the same fp32 terms without rounding worth the name."""
    return _per_list_f64(terms, offsets, entries, weights, False)


def bound(terms, offsets, entries, weights=None):
    """[N, d] fp64: (L - 1) 2^-24 sum |term| + one ulp of the result, L the list's length -- the first-order forward bound of
    a recursive fp32 sum (L - 1 additions, each within 2^-24 relative of a partial sum no larger than sum |term|), and the ulp
    for the terms of second order and the last rounding."""
    lengths = np.diff(np.asarray(offsets).astype(np.int64)).astype(np.float64)[:, None]
    mass = _per_list_f64(terms, offsets, entries, weights, True)
    result = np.abs(_per_list_f64(terms, offsets, entries, weights, False)).astype(F)
    return np.maximum(lengths - 1, 0) * U * mass + np.spacing(result).astype(np.float64)


# ----------------------------------------------------------------------------------------------------------------------
# the generator of the GPU tests, and the order-sensitivity of what it makes
# ----------------------------------------------------------------------------------------------------------------------
def make_idx(seed, B, E, N, hot=None, hot_count=0, empty=()):
    """[B, E] int32 in [0, N): uniform, then no entry on the sources ``empty``, then exactly ``hot_count`` entries of every
    shape on source ``hot``, at scattered entry numbers."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N, size=(B, E), dtype=np.int64)
    avoid = sorted(set(empty) | ({hot} if hot is not None else set()))
    if avoid:
        allowed = np.setdiff1d(np.arange(N), avoid)
        assert allowed.size > 0
        idx = allowed[rng.integers(0, allowed.size, size=(B, E))]
    if hot is not None:
        for b in range(B):
            idx[b, rng.choice(E, size=hot_count, replace=False)] = hot
    return idx.astype(np.int32)


def make_terms(seed, shape, bf16=False):
    """Standard normal fp32.  ``bf16``: values a bf16 holds, each scaled by a power of two from 2^-12 to 2^12 -- plain normal
    bf16 terms (8 significant bits, a narrow range) add up without any rounding in fp32, whatever the order."""
    rng = np.random.default_rng(seed)
    terms = rng.standard_normal(shape, dtype=F)
    if not bf16:
        return terms
    terms = terms * np.exp2(rng.integers(-12, 13, size=shape)).astype(F)
    bits = terms.view(np.uint32)
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) & np.uint32(0xFFFF0000)).view(F)      # round to nearest even at 8 bits


def make_weights(seed, shape):
    return np.random.default_rng(seed).uniform(0.0, 1.0, shape).astype(F)


def reversed_lists(offsets, entries):
    """The same lists, each in the opposite order."""
    offsets, entries = np.asarray(offsets).astype(np.int64), np.asarray(entries)
    src = np.repeat(np.arange(offsets.size - 1), np.diff(offsets))
    return entries[offsets[src] + offsets[src + 1] - 1 - np.arange(entries.size)]


def order_matters(terms, offsets, entries, weights=None, columns=8):
    """Do the lists summed backwards give other bits somewhere in the first ``columns`` columns?"""
    cut = np.ascontiguousarray(np.asarray(terms)[:, :columns])
    forward = list_sums(cut, offsets, entries, weights)
    backward = list_sums(cut, offsets, reversed_lists(offsets, entries), weights)
    return not np.array_equal(forward.view(np.int32), backward.view(np.int32))
