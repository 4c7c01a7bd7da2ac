"""The inverse-list builder nsdp_knn_invert and the older consumers of its lists -- nsdp_segment_sum_rows*, nsdp_scatter_cm_lists,
nsdp_three_interpolate_grad_lists -- held to their contract bit for bit: the lists are the stable sort of the entry numbers by
source index (tests/list_sum_ref.inverse_lists_ref), and every sum adds its terms in fp32, one after the other, in list order
(list_sum_ref.list_sums).  The C entries are called directly on outputs pre-filled with a sentinel; the consumers read lists
uploaded from the host reference, so no section depends on another.  Every case states the kernel form that ran (the variant
trace), and every exact comparison first asserts that its own inputs summed backwards give other bits -- a kernel that added in
another order could not pass by accident.

Forms on a 256-CU part (test_every_form_of_the_channel_major_reductions_is_covered): all of scatter_cm_lists<1|2|4|8>,
scatter_cm_lists_sliced<2,8|2,16|4,8>, three_interpolate_grad_lists<1|2|4|8> and three_interpolate_grad_sliced<4,8|2,16> are
reachable and run here."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

import list_sum_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_ci = ctypes.c_int
INT_SENTINEL, F_SENTINEL = -7, -777.0
KIB = 1024


class _Trace:
    """Context manager around nsdp_trace_*: ``names`` = the kernel variants launched inside."""

    def __enter__(self):
        from nsdp_amd import _lib
        self.L = _lib.lib()
        self.names = set()
        self.L.nsdp_trace_enable(1)
        return self

    def __exit__(self, *exc):
        self.L.nsdp_trace_enable(0)
        n = self.L.nsdp_trace_read(None, 0)
        buf = ctypes.create_string_buffer(n)
        self.L.nsdp_trace_read(buf, n)
        self.names = set(x for x in buf.value.decode().split("\n") if x)
        return False


def _num_cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, want):
    """torch.equal of a device result and a host array, with the worst difference in the message."""
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} elements differ, worst " \
                                      f"{float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()):.3e}"


# ----------------------------------------------------------------------------------------------------------------------
# a. nsdp_knn_invert
# ----------------------------------------------------------------------------------------------------------------------
def _invert(idx, N):
    """nsdp_knn_invert on idx [B, E] (host) -> offsets, entries (host) and the form that ran, 'lds' or 'global'."""
    from nsdp_amd import _lib
    L = _lib.lib()
    B, E = idx.shape
    d_idx = _dev(idx)
    off = torch.full((B, N + 1), INT_SENTINEL, dtype=torch.int32, device=DEV)
    ent = torch.full((B, E), INT_SENTINEL, dtype=torch.int32, device=DEV)
    with _Trace() as tr:
        _lib.check(L.nsdp_knn_invert(_lib.iptr(d_idx, "idx"), _ci(B), _ci(E), _ci(N), _lib.iptr(off), _lib.iptr(ent),
                                     _lib.stream_ptr()), "nsdp_knn_invert")
    torch.cuda.synchronize()
    names = [n for n in tr.names if n.startswith("knn_invert<")]
    assert len(names) == 1, tr.names
    return off.cpu().numpy(), ent.cpu().numpy(), names[0][len("knn_invert<"):-1]


def _form(E, N):
    """The entry's own rule: counters and entries of one shape in 148 KiB of LDS, or the entries in global memory."""
    return "lds" if (N + 1 + E) * 4 <= 148 * KIB else "global"


def _check_lists(idx, N, form):
    assert _form(idx.shape[1], N) == form                       # (the table states what the dispatch arithmetic gives)
    off, ent, ran = _invert(idx, N)
    assert ran == form
    want_off, want_ent = R.inverse_lists_ref(idx, N)
    assert np.array_equal(off, want_off)
    assert np.array_equal(ent, want_ent), f"{int((ent != want_ent).sum())} of {ent.size} entries differ"


@pytest.mark.parametrize("B,E,N,form", [
    (1, 1, 1, "lds"), (3, 259, 5, "lds"), (2, 4800, 700, "lds"),                       # small and ragged
    (2, 3000, 1023, "lds"), (2, 3000, 1024, "lds"), (2, 3000, 1025, "lds"),            # a scan thread owns 1 / 2 sources
    (1, 4000, 32768, "lds"), (1, 6000, 32768, "global"),                               # the source limit, either form
    (1, 35840, 2047, "lds"), (1, 35841, 2047, "global"),                               # the last LDS size, the first global one
    (2, 4096, 300, "lds"), (2, 36864, 2047, "global")])                                # E a multiple of the 1024 threads (3000, 35841: not)
def test_lists_are_the_stable_sort(B, E, N, form):
    _check_lists(R.make_idx(E + N, B, E, N), N, form)


def test_every_entry_on_one_source():
    E, N = 1000, 50
    idx = np.full((2, E), 17, dtype=np.int32)
    want_off, want_ent = R.inverse_lists_ref(idx, N)            # every other list empty, the one ascending
    assert np.array_equal(want_off, np.where(np.arange(N + 1) <= 17, 0, E).astype(np.int32)[None].repeat(2, 0))
    assert np.array_equal(want_ent, np.arange(E, dtype=np.int32)[None].repeat(2, 0))
    _check_lists(idx, N, "lds")


LONG = {"lds": (5000, 300), "global": (6000, 32768)}            # (E, N) with room for a 1025-entry list in either form


@pytest.mark.parametrize("form", ["lds", "global"])
def test_a_list_of_exactly_the_sorted_maximum(form):
    """1024 entries at scattered entry numbers: the longest list that is put in order -- every list ascending."""
    E, N = LONG[form]
    idx = R.make_idx(77, 2, E, N, hot=5, hot_count=1024)
    assert int((idx[1] == 5).sum()) == 1024 and not np.array_equal(np.nonzero(idx[1] == 5)[0], np.arange(1024))
    _check_lists(idx, N, form)


@pytest.mark.parametrize("form", ["lds", "global"])
def test_a_list_one_over_the_sorted_maximum(form):
    """1025 entries: that list is complete but in no promised order (include/nsdp_scatter.h); the offsets and every other list
    are the reference's."""
    E, N = LONG[form]
    idx = R.make_idx(78, 2, E, N, hot=5, hot_count=1025)
    assert _form(E, N) == form
    off, ent, ran = _invert(idx, N)
    assert ran == form
    want_off, want_ent = R.inverse_lists_ref(idx, N)
    assert np.array_equal(off, want_off)
    for b in range(2):
        lo, hi = int(off[b, 5]), int(off[b, 6])
        assert hi - lo == 1025
        ent[b, lo:hi] = np.sort(ent[b, lo:hi])
    assert np.array_equal(ent, want_ent)


# ----------------------------------------------------------------------------------------------------------------------
# b. segment sums
# ----------------------------------------------------------------------------------------------------------------------
SEG_B, SEG_N = 3, 53        # B N = 159: a multiple of neither the points per wave nor of four times them for any d below
SEG_D = [4, 8, 12, 20, 64, 120, 136, 200, 256]      # 16, 8, 5 (one idle lane), 3, 4, 2 points per wave; one from d = 132 up


@functools.lru_cache(maxsize=None)
def _segment_lists():
    """Every list length from 0 to 9 (the unroll-by-four tail) and one list of 300, other sources in every shape."""
    rng = np.random.default_rng(5)
    lengths = np.arange(SEG_N) % 10
    lengths[10] = 300
    idx = np.stack([rng.permutation(np.repeat(np.arange(SEG_N), np.roll(lengths, 7 * b))) for b in range(SEG_B)]).astype(np.int32)
    off, ent = R.inverse_lists_ref(idx, SEG_N)
    assert set(range(10)) | {300} == set(np.diff(off[0]).tolist())
    return idx, off, ent


@functools.lru_cache(maxsize=None)
def _segment_reference(d, bf16):
    """(terms as the kernel reads them, their list sums, exact sums, bounds), read-only."""
    _, off, ent = _segment_lists()
    host = R.make_terms(100 + d, (SEG_B, ent.shape[1], d), bf16=bf16)
    terms = torch.from_numpy(host)
    if bf16:
        terms = terms.to(torch.bfloat16)
        assert torch.equal(terms.float(), torch.from_numpy(host))          # (the generator's bf16 terms are bf16 values)
    for b in range(SEG_B):
        assert R.order_matters(host[b], off[b], ent[b])          # (before anything is launched on these inputs)
    out = tuple(np.stack([f(host[b], off[b], ent[b]) for b in range(SEG_B)]) for f in (R.list_sums, R.exact_sums, R.bound))
    for a in out:
        a.setflags(write=False)
    return (terms,) + out


def _segment_sum(src, off, ent, N, scale, addend, out):
    from nsdp_amd import _lib
    L = _lib.lib()
    B, E, d = src.shape
    name = "nsdp_segment_sum_rows" + ("_add" if addend is not None else "") + ("_bf16" if src.dtype is torch.bfloat16 else "")
    args = [ctypes.c_void_p(src.data_ptr()), _lib.iptr(off), _lib.iptr(ent), _ci(B), _ci(E), _ci(N), _ci(d), ctypes.c_float(scale)]
    args += [_lib.fptr(addend, "addend")] if addend is not None else []
    _lib.check(getattr(L, name)(*args, _lib.fptr(out), _lib.stream_ptr()), name)
    return out


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", SEG_D)
def test_segment_sums_add_in_list_order(d, bf16):
    _, off, ent = _segment_lists()
    terms, sums, exact, lim = _segment_reference(d, bf16)
    src, d_off, d_ent = terms.to(DEV), _dev(off), _dev(ent)
    add_host = R.make_terms(200 + d, (SEG_B, SEG_N, d))
    add = _dev(add_host)
    empty = np.diff(off, axis=1) == 0
    for scale in (1.0, -1.0):
        for addend in (None, add):
            out = torch.full((SEG_B, SEG_N, d), F_SENTINEL, device=DEV)
            got = _segment_sum(src, d_off, d_ent, SEG_N, scale, addend, out)
            want = sums * np.float32(scale)
            if addend is not None:
                want = want + add_host
            _same(got, want)
            rows = got.cpu().numpy()[empty]
            if addend is None:
                assert not rows.any() and (scale < 0 or not np.signbit(rows).any())          # (+0; -1 times +0 is -0)
            else:
                assert np.array_equal(rows, add_host[empty])
    # a general scale with the addend: the compiler may fuse scale * sum + addend (this file is built with contraction on), so
    # within the sum's bound and two ulp of |scale sum| + |addend| for the multiplication and the addition
    scale = np.float32(0.37)
    out = torch.full((SEG_B, SEG_N, d), F_SENTINEL, device=DEV)
    got = _segment_sum(src, d_off, d_ent, SEG_N, float(scale), add, out).cpu().numpy().astype(np.float64)
    want = np.float64(scale) * exact + add_host
    tol = np.float64(scale) * lim + 2 * np.spacing((np.abs(np.float64(scale) * exact) + np.abs(add_host)).astype(np.float32))
    err = np.abs(got - want)
    print(f"scale 0.37: worst error / tolerance {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all())


@pytest.mark.parametrize("d", [6, 260])
def test_segment_sums_refuse_other_row_lengths(d):
    from nsdp_amd import _lib
    _, off, ent = _segment_lists()
    d_off, d_ent = _dev(off), _dev(ent)
    add = torch.zeros(SEG_B, SEG_N, d, device=DEV)
    for dt in (torch.float32, torch.bfloat16):
        src = torch.ones(SEG_B, ent.shape[1], d, dtype=dt, device=DEV)
        for addend in (None, add):
            out = torch.full((SEG_B, SEG_N, d), F_SENTINEL, device=DEV)
            with pytest.raises(_lib.NsdpHipError, match="segment_sum_rows"):
                _segment_sum(src, d_off, d_ent, SEG_N, 1.0, addend, out)
            torch.cuda.synchronize()
            assert bool((out == F_SENTINEL).all())


def test_segment_sum_has_the_same_bits_from_either_builder():
    """hip_attention.segment_sum over the lists of the one-workgroup builder in its global form and of the many-workgroup
    builder: the same bits, the reference's."""
    from nsdp_amd import hip_attention as ha
    B, E, N, d = 1, 35841, 2047, 8
    idx = R.make_idx(9, B, E, N, hot=5, hot_count=600, empty=(0, N - 1))
    terms = R.make_terms(10, (B, E, d))
    off, ent = R.inverse_lists_ref(idx, N)
    assert R.order_matters(terms[0], off[0], ent[0])
    want = R.list_sums(terms[0], off[0], ent[0])[None]
    src, d_idx = _dev(terms).view(B, E, 1, d), _dev(idx).view(B, E, 1)
    with ha.invert_wide_mode("0"), _Trace() as tr:
        assert not ha._use_wide(B, E, N)
        one = ha.segment_sum(src, d_idx.clone(), N, 1.0)
    assert "knn_invert<global>" in tr.names
    with ha.invert_wide_mode("force"), _Trace() as tr:
        assert ha._use_wide(B, E, N)
        wide = ha.segment_sum(src, d_idx.clone(), N, 1.0)
    assert not [n for n in tr.names if n.startswith("knn_invert<")]
    assert torch.equal(one, wide)
    _same(wide, want)


# ----------------------------------------------------------------------------------------------------------------------
# c. channel-major reductions
# ----------------------------------------------------------------------------------------------------------------------
LDS_ROWS, LDS_MAX = 64 * KIB, 128 * KIB


def _whole_row_channels(row_bytes, B, C, cus):
    """Channels per workgroup of the whole-row kernels: what fits the LDS table, halved until 2 workgroups per CU exist."""
    ch = (LDS_ROWS if row_bytes <= LDS_ROWS else LDS_MAX) // row_bytes
    ch = 8 if ch >= 8 else 4 if ch >= 4 else 2 if ch >= 2 else 1
    while ch > 1 and B * -(-C // ch) < 2 * cus:
        ch >>= 1
    return ch


def _scatter_form(B, C, N, E, cus):
    """The dispatch arithmetic of nsdp_scatter_cm_lists."""
    if 4 * E > LDS_MAX:
        many = N > 8192
        four = not many and B * -(-C // 4) >= 2 * cus
        return f"scatter_cm_lists_sliced<{4 if four else 2},{16 if many else 8}>"
    return f"scatter_cm_lists<{_whole_row_channels(4 * E, B, C, cus)}>"


def _interp_form(B, c, n, m, cus):
    """The dispatch arithmetic of nsdp_three_interpolate_grad_lists."""
    if 4 * n > LDS_ROWS // 2:
        return "three_interpolate_grad_sliced<2,16>" if m > 8192 else "three_interpolate_grad_sliced<4,8>"
    return f"three_interpolate_grad_lists<{_whole_row_channels(4 * n, B, c, cus)}>"


def _slice_entries(form):
    """Entry numbers per slice of a sliced form: 128 KiB of LDS over its channels, three entries per element when interpolating."""
    ch = int(form[form.index("<") + 1])
    return LDS_MAX // 4 // ch * (3 if form.startswith("three") else 1)


# (B, C, N, E): every shape has a channel tail (C no multiple of the channels per workgroup), empty lists and a hot source
SCATTER_CASES = {
    "scatter_cm_lists<1>": [(2, 5, 97, 700), (1, 3, 5000, 32768)],       # too few rows for more; the longest whole row (128 KiB)
    "scatter_cm_lists<2>": [(4, 255, 97, 700)],
    "scatter_cm_lists<4>": [(4, 509, 97, 701)],                          # (E not a multiple of 4: the scalar staging)
    "scatter_cm_lists<8>": [(4, 1021, 97, 2048)],                        # (eight rows fill the 64 KiB table exactly)
    "scatter_cm_lists_sliced<2,8>": [(1, 3, 700, 32772), (2, 3, 700, 32769)],      # the first sliced rows: aligned; ragged with a last slice of 1
    "scatter_cm_lists_sliced<4,8>": [(256, 5, 64, 32772)],               # B ceil(C / 4) = 512 workgroups; a last slice of 4
    "scatter_cm_lists_sliced<2,16>": [(1, 3, 8193, 32769)],
}
# (B, c, n, m): 3 n entries
INTERP_CASES = {
    "three_interpolate_grad_lists<1>": [(2, 5, 233, 97)],
    "three_interpolate_grad_lists<2>": [(4, 255, 233, 97)],
    "three_interpolate_grad_lists<4>": [(4, 509, 234, 97)],
    "three_interpolate_grad_lists<8>": [(4, 1021, 2048, 300)],
    "three_interpolate_grad_sliced<4,8>": [(2, 5, 8193, 700), (1, 5, 8196, 700)],      # ragged, a last slice of 1 element; aligned
    "three_interpolate_grad_sliced<2,16>": [(1, 3, 16385, 8193)],
}
HOT = 5


def _hot_count(form, E):
    return 1100 if "sliced" in form or E > 8192 else 200          # (a sliced form: longer than it takes as ascending)


def _flat(cases):
    return [pytest.param(form, *shape, id=f"{form}-{'x'.join(map(str, shape))}") for form, shapes in cases.items() for shape in shapes]


def test_every_form_of_the_channel_major_reductions_is_covered():
    """The tables above name every form the two entries can dispatch, and on this part the arithmetic gives the named form for
    every shape (each case then asserts the trace).  All forms are reachable on a 256-CU part."""
    cus = _num_cus()
    assert set(SCATTER_CASES) == {f"scatter_cm_lists<{c}>" for c in (1, 2, 4, 8)} | {
        "scatter_cm_lists_sliced<2,8>", "scatter_cm_lists_sliced<2,16>", "scatter_cm_lists_sliced<4,8>"}
    assert set(INTERP_CASES) == {f"three_interpolate_grad_lists<{c}>" for c in (1, 2, 4, 8)} | {
        "three_interpolate_grad_sliced<4,8>", "three_interpolate_grad_sliced<2,16>"}
    for form, shapes in SCATTER_CASES.items():
        for shape in shapes:
            assert _scatter_form(*shape, cus) == form, (shape, cus)
    for form, shapes in INTERP_CASES.items():
        for shape in shapes:
            assert _interp_form(*shape, cus) == form, (shape, cus)


def _scatter(go, off, ent, N):
    """nsdp_scatter_cm_lists: go [B, C, E], lists [B, ..] (device) -> grad [B, C, N], trace names."""
    from nsdp_amd import _lib
    B, C, E = go.shape
    out = torch.full((B, C, N), F_SENTINEL, device=DEV)
    with _Trace() as tr:
        _lib.check(_lib.lib().nsdp_scatter_cm_lists(_lib.fptr(go, "grad_out"), _lib.iptr(off), _lib.iptr(ent), _ci(B), _ci(C), _ci(N),
                                                    _ci(E), _lib.fptr(out), _lib.stream_ptr()), "nsdp_scatter_cm_lists")
    return out, tr.names


def _interp(go, w, off, ent, m):
    """nsdp_three_interpolate_grad_lists: go [B, c, n], w [B, 3 n], lists over 3 n entries -> grad [B, c, m], trace names."""
    from nsdp_amd import _lib
    B, c, n = go.shape
    out = torch.full((B, c, m), F_SENTINEL, device=DEV)
    with _Trace() as tr:
        _lib.check(_lib.lib().nsdp_three_interpolate_grad_lists(_lib.fptr(go, "grad_out"), _lib.fptr(w, "weight"), _lib.iptr(off),
                                                                _lib.iptr(ent), _ci(B), _ci(c), _ci(n), _ci(m), _lib.fptr(out),
                                                                _lib.stream_ptr()), "nsdp_three_interpolate_grad_lists")
    return out, tr.names


def _cm_reference(go, off, ent, weights=None, sums=R.list_sums):
    """go [B, C, rows] channel-major; two index sets shared by the shapes of equal parity (lists [2, ..]), so one walk of a set's
    lists serves the channels of all its shapes -> [B, C, N]."""
    B, C, _ = go.shape
    N = off.shape[1] - 1
    want = np.empty((B, C, N), dtype=np.float32)
    for q in range(min(B, off.shape[0])):
        mine = go[q::off.shape[0]]
        terms = np.ascontiguousarray(mine.reshape(-1, mine.shape[2]).T)
        w = None if weights is None else weights[q]
        assert R.order_matters(terms, off[q], ent[q], w)         # (before anything is launched on these inputs)
        want[q::off.shape[0]] = sums(terms, off[q], ent[q], w).T.reshape(mine.shape[0], C, N)
    return want


def _cm_lists(seed, B, E, N, count, permute_hot=False):
    """Reference lists of min(B, 2) index sets, shape b reading set b % 2: host lists per set, device lists per shape."""
    sets = min(B, 2)
    idx = R.make_idx(seed, sets, E, N, hot=HOT, hot_count=count, empty=(0, N - 1))
    off, ent = R.inverse_lists_ref(idx, N)
    if permute_hot:
        rng = np.random.default_rng(seed + 1)
        for q in range(sets):
            lo, hi = off[q, HOT], off[q, HOT + 1]
            ent[q, lo:hi] = rng.permutation(ent[q, lo:hi])
    pick = np.arange(B) % sets
    return off, ent, _dev(off[pick]), _dev(ent[pick])


@pytest.mark.parametrize("form,B,C,N,E", _flat(SCATTER_CASES))
def test_scatter_cm_lists_adds_in_list_order(form, B, C, N, E):
    off, ent, d_off, d_ent = _cm_lists(E + C, B, E, N, _hot_count(form, E))
    go = R.make_terms(E + N, (B, C, E))
    want = _cm_reference(go, off, ent)
    got, names = _scatter(_dev(go), d_off, d_ent, N)
    assert names == {_scatter_form(B, C, N, E, _num_cus())} == {form}
    _same(got, want)
    assert not want[:, :, [0, N - 1]].any() and not got[:, :, [0, N - 1]].any()              # the empty lists


@pytest.mark.parametrize("form,B,c,n,m", _flat(INTERP_CASES))
def test_three_interpolate_grad_lists_adds_in_list_order(form, B, c, n, m):
    off, ent, d_off, d_ent = _cm_lists(n + c, B, 3 * n, m, _hot_count(form, 3 * n))
    go, w = R.make_terms(n + m, (B, c, n)), R.make_weights(n + m + 1, (B, 3 * n))
    want = _cm_reference(go, off, ent, weights=w[: off.shape[0]])
    w_dev = _dev(w[np.arange(B) % off.shape[0]])                   # (the weights belong to the index set)
    got, names = _interp(_dev(go), w_dev, d_off, d_ent, m)
    assert names == {_interp_form(B, c, n, m, _num_cus())} == {form}
    _same(got, want)
    assert not got[:, :, [0, m - 1]].any()


@pytest.mark.parametrize("kind", ["scatter", "interpolate"])
def test_sliced_forms_take_a_long_list_slice_by_slice(kind):
    """A list over 1024 entries in scrambled order (what the one-workgroup builder may leave): the sliced kernels add it slice
    after slice, in stored order inside a slice (list_sum_ref.sliced_list_sums) -- not in the stored order of the whole list,
    which this data tells apart.  (Ascending, as the many-workgroup builder writes it, it is list order: the cases above.)"""
    if kind == "scatter":
        form, (B, C, N, E) = "scatter_cm_lists_sliced<2,8>", (2, 3, 700, 32769)
        rows, entries = E, E
    else:
        form, (B, C, rows, N) = "three_interpolate_grad_sliced<4,8>", (2, 5, 3 * 8192 + 1, 700)      # four slices, the last of 1
        entries = 3 * rows
    off, ent, d_off, d_ent = _cm_lists(31, B, entries, N, 1100, permute_hot=True)
    go = R.make_terms(32, (B, C, rows))
    w = R.make_weights(33, (B, entries)) if kind == "interpolate" else None
    rule = functools.partial(R.sliced_list_sums, slice=_slice_entries(form))
    want = _cm_reference(go, off, ent, weights=w, sums=rule)
    stored = _cm_reference(go, off, ent, weights=w)
    assert not np.array_equal(want[:, :, HOT], stored[:, :, HOT])
    assert np.array_equal(np.delete(want, HOT, axis=2), np.delete(stored, HOT, axis=2))
    if kind == "scatter":
        got, names = _scatter(_dev(go), d_off, d_ent, N)
    else:
        got, names = _interp(_dev(go), _dev(w), d_off, d_ent, N)
    assert names == {form}
    _same(got, want)


# ----------------------------------------------------------------------------------------------------------------------
# through the Python layer
# ----------------------------------------------------------------------------------------------------------------------
def test_grouping_operation_backward_is_the_direct_call():
    from nsdp_amd import hip_attention as ha, pointnet2_utils as pu
    B, C, N, NP, NS = 2, 6, 64, 16, 8
    idx = R.make_idx(41, B, NP * NS, N, hot=HOT, hot_count=30, empty=(0, N - 1))
    go = R.make_terms(42, (B, C, NP * NS))
    off, ent = R.inverse_lists_ref(idx, N)
    want = np.stack([R.list_sums(np.ascontiguousarray(go[b].T), off[b], ent[b]).T for b in range(B)])
    assert all(R.order_matters(np.ascontiguousarray(go[b].T), off[b], ent[b]) for b in range(B))
    d_idx = _dev(idx).view(B, NP, NS)
    feats = torch.zeros(B, C, N, device=DEV, requires_grad=True)
    out = pu.grouping_operation(feats, d_idx)
    with _Trace() as tr:
        out.backward(_dev(go).view(B, C, NP, NS))
    assert [n for n in tr.names if n.startswith("scatter_cm_lists<")], tr.names
    d_off, d_ent = ha.inverse_lists(d_idx, N)
    direct, _ = _scatter(_dev(go), d_off, d_ent, N)
    assert torch.equal(feats.grad, direct)
    _same(feats.grad, want)


def test_three_interpolate_backward_is_the_direct_call():
    from nsdp_amd import hip_attention as ha, pointnet2_utils as pu
    B, c, m, n = 2, 6, 50, 40
    idx = R.make_idx(43, B, 3 * n, m, hot=HOT, hot_count=30, empty=(0, m - 1))
    go, w = R.make_terms(44, (B, c, n)), R.make_weights(45, (B, 3 * n))
    off, ent = R.inverse_lists_ref(idx, m)
    want = np.stack([R.list_sums(np.ascontiguousarray(go[b].T), off[b], ent[b], w[b]).T for b in range(B)])
    assert all(R.order_matters(np.ascontiguousarray(go[b].T), off[b], ent[b], w[b]) for b in range(B))
    d_idx, d_w = _dev(idx).view(B, n, 3), _dev(w).view(B, n, 3)
    feats = torch.zeros(B, c, m, device=DEV, requires_grad=True)
    out = pu.three_interpolate(feats, d_idx, d_w)
    with _Trace() as tr:
        out.backward(_dev(go))
    assert [x for x in tr.names if x.startswith("three_interpolate_grad_lists<")], tr.names
    d_off, d_ent = ha.inverse_lists(d_idx, m)
    direct, _ = _interp(_dev(go), _dev(w), d_off, d_ent, m)
    assert torch.equal(feats.grad, direct)
    _same(feats.grad, want)
