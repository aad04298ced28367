"""The committee axes of the mc side -- class count, member count, dtype, strides
and alignment -- against the CPU oracle (tests/test_oracle_axes.py pins the
oracle itself to numpy / scipy at every class count).

Every mc / mix / batched / chunked entry point reads the committee through
CommitteeSrc / MemberLoad (C in {2, 3, 4, 8}: csrc/ce_src.hpp, ce_device.hpp)
or through the wide kernels (every other C up to 2048: csrc/ce_wide.hpp,
ce_wide_stream.hpp).  This module sweeps

* every wide C in 1..2048 for f32, f64 and bf16, on the vector kernels and --
  through views that break their 16-byte rule -- on the strided ones;
* a short list of wide C next to every threshold (the 8-accumulator block, the
  128-element leaf, 64 / 128 chunks per row, NPL at 512 / 1024, the last C)
  through the streaming, block-list, bitmap, member-major and chunked paths;
* dtype x C x M x layout x view class for the narrow C, at a single-block pool,
  a small multi-block pool and a streaming pool;
* the error contract at the ends of the class axis.

Bar: bit for bit (ENT_TOL_ULP = 0 in test_gpu_parity.py).  f64 results compare
as uint64 patterns with NaN matching NaN; indices compare against
oracle.ce_oracle.canonical_order.

Where the library names the kernel it launched (ce_last_kernel()), the
CommitteeSrc<dtype, C, vec> arguments in the name are compared with what the
test works out from the tensor's own data_ptr() and strides (vec_rule below,
which restates the rule, it does not read it from the library), so the matrix
cannot silently collapse onto the scalar loads -- or take vector loads on a
view that does not allow them."""
import re

import numpy as np
import pytest

from axes_common import bf16_bits, first_diff, same_bits

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DTS = ("f32", "f64", "bf16")
EB = {"f32": 4, "f64": 8, "bf16": 2}
CODE = {"f32": 0, "f64": 1, "bf16": 2}  # the dtype codes in the kernel names (kF32, kF64, kBF16)
NARROW_C = (2, 3, 4, 8)
# the CommitteeSrc<dtype, C, true> instantiations (with_committee, csrc/ce_dispatch.hpp)
HAS_VEC = {("f32", 4), ("f32", 8), ("f64", 2), ("f64", 4), ("f64", 8), ("bf16", 4), ("bf16", 8)}

SEEN_SRC = set()      # (dtype, C, vec) of every CommitteeSrc named by ce_last_kernel()
SEEN_KERNELS = set()  # every distinct ce_last_kernel() string
SEEN_M = set()        # member counts the narrow matrix ran
SEEN_WIDE = set()     # (dtype, C, "vec" | "strided") of the wide sweeps


@pytest.fixture(scope="module")
def ce():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ce_amd
    import ce_amd.ops

    ce_amd.load()
    return ce_amd


def last_kernel(ce):
    k = ce._lib.load().ce_last_kernel().decode()
    SEEN_KERNELS.add(k)
    return k


# ---------------------------------------------------------------------------
# committees as views of one flat parent buffer, the same view on both sides
# ---------------------------------------------------------------------------
def draw(rng, n, dt):
    """n positive values in (0.001, 1.001) in the host form of dtype dt (bf16: uint16 bit patterns).
    Rows of them are unnormalised; bf16 keeps 8 bits, so bf16 pools hold many exact entropy ties."""
    x = rng.random(n) + 1e-3
    if dt == "f64":
        return x
    x = x.astype(np.float32)
    return x if dt == "f32" else bf16_bits(x)


def enc(dt, v):
    """The host representation of the value v in dtype dt."""
    return bf16_bits(np.float32(v)).reshape(-1)[0] if dt == "bf16" else v


def to_dev(host, dt):
    if dt == "bf16":
        return torch.from_numpy(host.view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(host).cuda()


def hview(host, base, shape, strides):
    """The numpy view (element strides) of a flat host buffer."""
    return np.lib.stride_tricks.as_strided(host[base:], shape, tuple(s * host.itemsize for s in strides))


def items_of(v, layout):
    """[N, M, C] indexing of a committee view of either layout."""
    return v if layout == "NMC" else v.transpose(1, 0, 2)


def strides_of(t, layout):
    """(sN, sM, sC) in elements."""
    s = t.stride()
    return (s[0], s[1], s[2]) if layout == "NMC" else (s[1], s[0], s[2])


def vec_rule(t, layout, dt):
    """Whether CommitteeSrc may take vector loads on this tensor: unit class
    stride, whole vectors per row (C % 4, f64: C % 2), and the base pointer and
    both pitches multiples of the vector's bytes (16, bf16: 8)."""
    C = t.shape[2]
    sN, sM, sC = strides_of(t, layout)
    eb, vb = EB[dt], (8 if dt == "bf16" else 16)
    return (sC == 1 and C % (2 if dt == "f64" else 4) == 0 and t.data_ptr() % vb == 0 and (sN * eb) % vb == 0
            and (sM * eb) % vb == 0)


def wide_rule(t, layout, dt):
    """Whether the wide kernels may take 16-byte chunks: unit class stride, rows
    of whole chunks, base pointer and both pitches multiples of 16 bytes."""
    C = t.shape[2]
    sN, sM, sC = strides_of(t, layout)
    eb = EB[dt]
    return (sC == 1 and (C * eb) % 16 == 0 and t.data_ptr() % 16 == 0 and (sN * eb) % 16 == 0
            and (sM * eb) % 16 == 0)


def npl_of(C):
    return 8 if C <= 512 else (16 if C <= 1024 else 32)


SRC_RE = re.compile(r"CommitteeSrc<(\d+), (\d+), (true|false)>")


def check_src(ce, t, layout, dt, what, mix=False):
    """After a selection on committee t: if the library named its kernel, the
    first CommitteeSrc in the name must carry this dtype, this C and the vec
    this view allows.  A mix names the committee's source only from its
    one-block kernel (the table's second); past it the last kernel named is the
    hc table's own pass."""
    k = last_kernel(ce)
    if mix and not k.startswith("ce::k_select_tiles<"):
        return
    m = SRC_RE.search(k)
    if m is None:
        if "k_stream_nmc<" in k:  # the LDS-DMA tiles: dense, aligned committees only
            assert vec_rule(t, layout, dt), (what, k)
        return
    got = (int(m.group(1)), int(m.group(2)), m.group(3) == "true")
    want = (CODE[dt], t.shape[2], vec_rule(t, layout, dt))
    assert got == want, (what, k, want, t.data_ptr() % 16, strides_of(t, layout))
    SEEN_SRC.add((dt, t.shape[2], got[2]))


def check_wide_kernel(ce, t, layout, dt, what):
    """After a streaming selection (q <= 64) on a wide committee: the pipelined
    vector kernel exactly when the view keeps the 16-byte rule."""
    k = last_kernel(ce)
    C = t.shape[2]
    if wide_rule(t, layout, dt):
        assert k.startswith("ce::k_stream_wide2<%d, " % CODE[dt]), (what, k)
    else:
        assert k == "ce::k_stream_wide<%d, %d, false>" % (CODE[dt], npl_of(C)), (what, k)
    return k


def assert_bits(got, exp, what):
    assert same_bits(got, exp), (what,) + first_diff(got, exp)


def want_selection(ent, q, keep=None):
    from oracle import ce_oracle as O

    if keep is None:
        order = O.canonical_order(ent, q)
    else:
        order = keep[O.canonical_order(ent[keep], q)]
    return ent[order], order


def assert_selection(got, ent, q, what, keep=None):
    """(vals, idx) host arrays of q slots: the oracle's order and entropies, then padding."""
    vals, idx = got
    wv, wi = want_selection(ent, q, keep)
    n = len(wi)
    assert np.array_equal(idx[:n], wi), (what, idx[:8].tolist(), wi[:8].tolist())
    assert (idx[n:] == -1).all() and np.isnan(vals[n:]).all(), what
    assert_bits(vals[:n], wv, what)


def host_sel(sel):
    return sel[0].cpu().numpy(), sel[1].cpu().numpy()


def bitmap_every_third(ce, N):
    ex = ce.ops.excl_bitmap(N, "cuda")
    ce.ops.mark_selected(ex, N, torch.arange(0, N, 3, device="cuda"))
    return ex, np.flatnonzero(np.arange(N) % 3 != 0)


def sprinkle(rng, it, dt):
    """Special items into an [N, M, C] host view: a NaN member value, an all-zero
    row (0 / 0), a row of -0.0, a -0.0 class, a negative value, +inf, and three
    exact duplicates of one item (ties the lowest position breaks)."""
    N, M, C = it.shape
    k = rng.permutation(N)[:10]
    it[k[0], M - 1, C - 1] = enc(dt, np.nan)
    it[k[1]] = enc(dt, 0.0)
    it[k[2]] = enc(dt, -0.0)
    it[k[3], :, 0] = enc(dt, -0.0)
    it[k[4], 0, C // 2] = enc(dt, -0.05)
    it[k[5], 0, 0] = enc(dt, np.inf)
    it[k[7]] = it[k[6]]
    it[k[8]] = it[k[6]]
    it[k[9]] = it[k[6]]


# ---------------------------------------------------------------------------
# 2. every wide class count
# ---------------------------------------------------------------------------
WIDE_CS = [C for C in range(1, 2049) if C not in NARROW_C]
WIDE_MS = (1, 2, 3, 4, 5, 8)
N_ENT, N_SEL, Q_SEL = 9, 37, 5
WIDE_BUF = 37 * 8 * 2049 * 2 + 64  # the largest view of the sweep (sC = 2 / pitch C + 1, M = 8, N = 37)
_WIDE = {}


def wide_m(C):
    """The member count of class count C: through WIDE_MS as C advances, shifted once per period of every
    kernel-choosing rule (C % 2, 4, 8, 16) so each residue class of C meets every M."""
    return WIDE_MS[(C + C // 6 + C // 16) % 6]


def wide_buffer(dt):
    """One buffer of values per dtype for the whole sweep (host, device): every C takes views of it."""
    if dt not in _WIDE:
        host = draw(np.random.default_rng(7 + CODE[dt]), WIDE_BUF, dt)
        _WIDE[dt] = (host, to_dev(host, dt))
    return _WIDE[dt]


def wide_view(dt, C, M, N, kind):
    """(base, shape, strides) of an item-major [N, M, C] view: 'dense' at a
    16-byte-aligned base that moves with C, or one of the three views that break
    the 16-byte rule of a C whose dense rows keep it."""
    per16 = 16 // EB[dt]
    if kind == "dense":
        return (C % 5) * per16, (N, M, C), (M * C, C, 1)
    if kind == "base+1":  # flat[1:] as [N, M, C]
        return 1, (N, M, C), (M * C, C, 1)
    if kind == "pitch+1":  # member pitch C + 1
        return 0, (N, M, C), (M * (C + 1), C + 1, 1)
    assert kind == "sC2"
    return 0, (N, M, C), (2 * M * C, 2 * C, 2)


def wide_cases(dt, mode):
    """[(C, M, kind)]: mode 'dense' every wide C; mode 'strided' every C whose
    dense rows are whole 16-byte chunks, cycling through the three breaking views."""
    if mode == "dense":
        return [(C, wide_m(C), "dense") for C in WIDE_CS]
    out = []
    for C in WIDE_CS:
        if (C * EB[dt]) % 16 == 0:
            out.append((C, wide_m(C), ("base+1", "pitch+1", "sC2")[len(out) % 3]))
    return out


def test_wide_sweep_plan():
    """The sweep's own coverage (host arithmetic; it runs with the GPU tests it
    describes): per dtype, both the vector and the strided kernel meet every M
    of WIDE_MS in every NPL band, and every breaking view meets every band."""
    for dt in DTS:
        seen = {(npl_of(C), (C * EB[dt]) % 16 == 0, M) for C, M, _ in wide_cases(dt, "dense")}
        for npl in (8, 16, 32):
            for vec in (True, False):
                assert {M for n, v, M in seen if n == npl and v == vec} == set(WIDE_MS), (dt, npl, vec)
        kinds = {(npl_of(C), k) for C, _, k in wide_cases(dt, "strided")}
        assert kinds == {(n, k) for n in (8, 16, 32) for k in ("base+1", "pitch+1", "sC2")}, dt
        assert max(b + (s[0] - 1) * st[0] + (s[1] - 1) * st[1] + (s[2] - 1) * st[2] + 1
                   for C, M, k in wide_cases(dt, "dense") + wide_cases(dt, "strided")
                   for b, s, st in [wide_view(dt, C, M, N_SEL, k)]) <= WIDE_BUF


@pytest.mark.parametrize("mode", ["dense", "strided"])
@pytest.mark.parametrize("dt", DTS)
def test_wide_every_class_count(ce, dt, mode):
    """Every C in 1..2048 outside {2, 3, 4, 8} (mode 'strided': every C whose
    dense rows pass the 16-byte rule, as a view that breaks it): the entropies
    of N = 9 items (k_wide_entropy_v: three 4-wave blocks, the last ragged) and
    select_mc(q = 5) over N = 37 (the wide stream), M rotating through
    {1, 2, 3, 4, 5, 8}, all views of one buffer.  The launches of the whole
    sweep are queued first and read back once."""
    from oracle import ce_oracle as O

    host, devb = wide_buffer(dt)
    cases = wide_cases(dt, mode)
    ents, vals, idxs, want = [], [], [], []
    for C, M, kind in cases:
        base, shape, strides = wide_view(dt, C, M, N_SEL, kind)
        P = devb.as_strided(shape, strides, base)
        vec = wide_rule(P, "NMC", dt)
        assert vec == (mode == "dense" and (C * EB[dt]) % 16 == 0), (C, kind)
        ents.append(ce.ops.committee_entropy(P[:N_ENT], "NMC"))
        v, i = ce.ops.select_mc(P, Q_SEL, "NMC")
        check_wide_kernel(ce, P, "NMC", dt, (dt, C, M, kind))
        vals.append(v)
        idxs.append(i)
        want.append(O.oracle_committee_entropy(hview(host, base, shape, strides), "NMC"))
        SEEN_WIDE.add((dt, C, "vec" if vec else "strided"))
    ents = torch.stack(ents).cpu().numpy()
    vals, idxs = torch.stack(vals).cpu().numpy(), torch.stack(idxs).cpu().numpy()
    bad = []
    for r, (C, M, kind) in enumerate(cases):
        if not same_bits(ents[r], want[r][:N_ENT]):
            bad.append(("ent", C, M, kind) + first_diff(ents[r], want[r][:N_ENT]))
        wv, wi = want_selection(want[r], Q_SEL)
        if not (np.array_equal(idxs[r], wi) and same_bits(vals[r], wv)):
            bad.append(("select", C, M, kind, idxs[r].tolist(), wi.tolist()))
    assert not bad, (len(bad), bad[:6])


EDGE_CS = (1, 5, 7, 9, 15, 17, 127, 128, 129, 255, 256, 257, 260, 504, 511, 512, 513, 520, 1023, 1024, 1025, 1032,
           2040, 2047, 2048)
EDGE_MS = (4, 3, 2, 5, 8, 1)


def edge_n(M, C):
    """Items of an edge pool: about 1M elements, 130..3001 items, never a whole number of 64-item runs
    (nor one item past it)."""
    N = max(130, min(3001, 1_000_000 // (M * C)))
    return N + 2 if N % 64 < 2 else N


@pytest.mark.parametrize("C", EDGE_CS)
def test_wide_edges_deep_paths(ce, C):
    """Class counts next to every threshold of the wide kernels -- the n < 8
    row sum, the 8-accumulator block (15, 17), the 128-element leaf (127..129,
    255..257), 64 and 128 16-byte chunks per row (f64 128 / 256 / 260, f32 256 /
    260 / 512 / 520, bf16 504 / 512 / 520 / 1024 / 1032), NPL at 512 / 1024,
    and the last C -- for all three dtypes (M rotating with C and dtype) through
    the paths where a wave handles several items: select_mc at q = 10 (the
    stream) and q = 65 (block lists), with an exclusion bitmap, from a
    member-major copy, and as an MCChunkJob of two unequal chunks.

    Pool size.  The stream launches grid = min(resident blocks, ceil(N / 64))
    blocks of 4 waves (pool_blocks, stream_grid), W = 4 * grid waves.
    k_stream_wide2 deals items round-robin (wave g takes g, g + W, ...): every
    wave takes >= floor(N / W) items, and W <= 4 * ceil(N / 64) makes that >= 2
    for any N >= 16; at the N used here (130..3001, ~1M elements, N * M * C <=
    8M) a wave pipelines 8..16 items.  k_stream_wide gives a wave a run of
    per_wave = 64 * ceil(ceil(N / W) / 64) = 64 items, so the first ceil(N / 64)
    waves work and N % 64 >= 2 leaves the last of them a ragged run of at least
    two (filling all W waves of the strided kernel takes N > 64 * (W - 1):
    test_wide_strided_full_grid)."""
    from oracle import ce_oracle as O

    ci = EDGE_CS.index(C)
    for di, dt in enumerate(DTS):
        M = EDGE_MS[(ci + di) % len(EDGE_MS)]
        N = edge_n(M, C)
        assert N * M * C <= 8_000_000 and N % 64 >= 2
        rng = np.random.default_rng(1000 * C + di)
        host = draw(rng, N * M * C, dt)
        hv = hview(host, 0, (N, M, C), (M * C, C, 1))
        sprinkle(rng, hv, dt)
        ent = O.oracle_committee_entropy(hv, "NMC")
        P = to_dev(host, dt).view(N, M, C)
        what = (dt, C, M, N)
        vec = wide_rule(P, "NMC", dt)
        assert vec == ((C * EB[dt]) % 16 == 0)
        assert_selection(host_sel(ce.ops.select_mc(P, 10, "NMC")), ent, 10, what + ("q10",))
        check_wide_kernel(ce, P, "NMC", dt, what)
        assert_selection(host_sel(ce.ops.select_mc(P, 65, "NMC")), ent, 65, what + ("q65",))
        ex, keep = bitmap_every_third(ce, N)
        try:
            got = host_sel(ce.ops.select_mc(P, 10, "NMC", excl=ex))
        except ce._lib.CEError as e:
            # the one refusal test_gpu_dispatch_pins.py allows: k_stream_wide takes no bitmap (today the
            # ladder answers such a call from the block lists instead, and the answer is checked)
            assert not vec and e.code == ce._lib.CE_EUNSUPPORTED, (what, e)
        else:
            assert_selection(got, ent, 10, what + ("excl",), keep)
            if vec:
                check_wide_kernel(ce, P, "NMC", dt, what + ("excl",))
        assert_selection(host_sel(ce.ops.select_mc(P, 65, "NMC", excl=ex)), ent, 65, what + ("excl q65",), keep)
        Pm = P.permute(1, 0, 2).contiguous()
        assert_selection(host_sel(ce.ops.select_mc(Pm, 10, "MNC")), ent, 10, what + ("MNC",))
        check_wide_kernel(ce, Pm, "MNC", dt, what + ("MNC",))
        cut = N // 3 + 1
        job = ce.ops.MCChunkJob(10, "NMC")
        job.add(P[:cut])
        job.add(P[cut:])
        assert_selection(host_sel(job.result()), ent, 10, what + ("chunks",))


@pytest.mark.parametrize("C,M,dt", [(1, 8, "f32"), (5, 3, "bf16"), (7, 4, "f64"), (9, 3, "f32"), (15, 2, "bf16"),
                                    (17, 1, "f64")])
def test_wide_strided_full_grid(ce, C, M, dt):
    """k_stream_wide with a pool long enough for every wave of its grid: with the
    1024 blocks pool_blocks allows (4096 waves of 64-item runs) N = 4096 * 64 - 30
    gives every wave 64 items and the last one 34; on a smaller resident grid the
    runs grow to 128 and the trailing waves idle.  Only small odd C fit 8M elements."""
    from oracle import ce_oracle as O

    N = 4096 * 64 - 30
    assert N * M * C <= 8_000_000
    rng = np.random.default_rng(C)
    host = draw(rng, N * M * C, dt)
    hv = hview(host, 0, (N, M, C), (M * C, C, 1))
    sprinkle(rng, hv, dt)
    ent = O.oracle_committee_entropy(hv, "NMC")
    P = to_dev(host, dt).view(N, M, C)
    for q in (10, 65):
        assert_selection(host_sel(ce.ops.select_mc(P, q, "NMC")), ent, q, (dt, C, M, q))
        if q == 10:
            assert check_wide_kernel(ce, P, "NMC", dt, (dt, C, M)).startswith("ce::k_stream_wide<")


# ---------------------------------------------------------------------------
# 3. the narrow-C committee source matrix
# ---------------------------------------------------------------------------
NARROW_MS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 20, 33)
LAYOUTS = ("NMC", "MNC")
VIEWS = ("contig", "base+1", "item+1", "vecpad", "sC2")


def narrow_view(dt, layout, view, N, M, C):
    """(base, shape, strides, elements) of a committee view in a flat buffer.
    The inner axis is the member (NMC) or the item (MNC):
      contig   dense;
      base+1   dense, starting one element into the buffer;
      item+1   the item pitch one element longer: breaks the vector rule;
      vecpad   the inner and the outer pitch each padded by one whole vector
               (16 bytes; bf16: 8): the rule holds, the strides are not dense;
      sC2      every second class."""
    ve = (8 if dt == "bf16" else 16) // EB[dt]
    sC = 2 if view == "sC2" else 1
    a = b = 0  # padding of the inner / outer pitch
    if view == "item+1":
        a, b = (0, 1) if layout == "NMC" else (1, 0)
    elif view == "vecpad":
        a = b = ve
    n_in, n_out = (M, N) if layout == "NMC" else (N, M)
    s_in = C * sC + a
    s_out = n_in * s_in + b
    base = 1 if view == "base+1" else 0
    return base, (n_out, n_in, C), (s_out, s_in, sC), base + n_out * s_out


def narrow_pool(seed, dt, layout, view, N, M, C):
    """(device committee, host view, oracle entropies, oracle means) of one
    seeded pool with the special items sprinkled in."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(seed)
    base, shape, strides, n = narrow_view(dt, layout, view, N, M, C)
    host = draw(rng, n, dt)
    hv = hview(host, base, shape, strides)
    sprinkle(rng, items_of(hv, layout), dt)
    ent, mean = O.oracle_committee_entropy(hv, layout, want_mean=True)
    P = to_dev(host, dt).as_strided(shape, strides, base)
    assert vec_rule(P, layout, dt) == ((dt, C) in HAS_VEC and view in ("contig", "vecpad")), (dt, layout, view, M, C)
    SEEN_M.add(M)
    return P, hv, ent, mean


_SINGLE_DONE = set()


def run_single_block(ce, dt, view):
    """The full cross C x M x layout of one (dtype, view class) at N = 257."""
    N, q = 257, 10
    runs = []
    for C in NARROW_C:
        for M in NARROW_MS:
            for layout in LAYOUTS:
                seed = (((C * 64 + M) * 2 + (layout == "MNC")) * 8 + VIEWS.index(view)) * 4 + CODE[dt]
                P, _, ent, mean = narrow_pool(seed, dt, layout, view, N, M, C)
                e, m = ce.ops.committee_entropy(P, layout, return_mean=True)
                v, i = ce.ops.select_mc(P, q, layout)
                check_src(ce, P, layout, dt, (dt, view, C, M, layout))
                runs.append(((C, M, layout), e, m, v, i, ent, mean))
    bad = []
    for tag, e, m, v, i, ent, mean in runs:  # one read-back pass after every launch is queued
        e, m, v, i = e.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), i.cpu().numpy()
        if not same_bits(m, mean):
            bad.append(("mean", tag) + first_diff(m, mean))
        if not same_bits(e, ent):
            bad.append(("ent", tag) + first_diff(e, ent))
        wv, wi = want_selection(ent, q)
        if not (np.array_equal(i, wi) and same_bits(v, wv)):
            bad.append(("select", tag, i.tolist(), wi.tolist()))
    assert not bad, (dt, view, len(bad), bad[:6])
    _SINGLE_DONE.add((dt, view))


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("dt", DTS)
def test_narrow_matrix_single_block(ce, dt, view):
    """dtype x C in {2, 3, 4, 8} x M in NARROW_MS x {NMC, MNC} x view class at
    N = 257 (one block, a ragged last wave): committee_entropy's means and
    entropies (k_entropy) and select_mc at q = 10 (k_select_tiles: rows_small
    with M below, at and above its batch), every pool with the special items."""
    run_single_block(ce, dt, view)


def reduced_cases():
    """[(dt, view, C, M, layout)]: every (dtype, C, view class) once, M and the layout rotating so that
    every M of NARROW_MS appears (13 and the 4 class counts are coprime: M meets every C)."""
    out = []
    for vi, view in enumerate(VIEWS):
        for di, dt in enumerate(DTS):
            for ci, C in enumerate(NARROW_C):
                i = len(out)
                out.append((dt, view, C, NARROW_MS[(i + 5 * vi) % len(NARROW_MS)], LAYOUTS[(ci + di + vi) % 2]))
    return out


def ragged_users(N):
    """Users of 1, 63, 1, 635, 0 (empty), then the rest in two unequal parts."""
    return np.array([0, 1, 64, 65, 700, 700, 700 + (N - 700) * 2 // 5, N], np.int64)


@pytest.mark.parametrize("view", VIEWS)
@pytest.mark.parametrize("dt", DTS)
def test_narrow_reduced_multi_block(ce, dt, view):
    """One M and layout per (dtype, C, view class) -- every M of the list appears
    in the set -- at N = 5000 (the small-pool blocks and their wave merge, or the
    stream for the larger committees) and N = 70 001 (the streaming kernels):
    select_mc at q = 10 and 65, with an exclusion bitmap, select_batched over
    ragged users with an empty one, and for C = 4 select_mix with a small hc
    table; every pool with the special items."""
    from oracle import ce_oracle as O

    cases = [c for c in reduced_cases() if c[0] == dt and c[1] == view]
    assert sorted(c[2] for c in cases) == list(NARROW_C)
    assert {c[3] for c in reduced_cases()} == set(NARROW_MS)
    votes = np.random.default_rng(11).integers(-1, 4, (300, 30)).astype(np.int8)
    H = O.oracle_vote_table(votes)[0]
    ent_h = O.oracle_table_entropy(H)
    Hd = torch.from_numpy(H).cuda()
    for _, _, C, M, layout in cases:
        for N in (5000, 70_001):
            what = (dt, view, C, M, layout, N)
            P, _, ent, _ = narrow_pool(N + 31 * C + M, dt, layout, view, N, M, C)
            for q in (10, 65):
                assert_selection(host_sel(ce.ops.select_mc(P, q, layout)), ent, q, what + (q,))
                check_src(ce, P, layout, dt, what + (q,))
            ex, keep = bitmap_every_third(ce, N)
            assert_selection(host_sel(ce.ops.select_mc(P, 10, layout, excl=ex)), ent, 10, what + ("excl",), keep)
            check_src(ce, P, layout, dt, what + ("excl",))
            offs = ragged_users(N)
            bv, bi = host_sel(ce.ops.select_batched(P, torch.from_numpy(offs).cuda(), 10, layout))
            check_src(ce, P, layout, dt, what + ("batched",))
            for u in range(len(offs) - 1):
                assert_selection((bv[u], bi[u]), ent[offs[u]:offs[u + 1]], 10, what + ("user", u))
            if C == 4:
                got = host_sel(ce.ops.select_mix(P, Hd, 10, layout))
                check_src(ce, P, layout, dt, what + ("mix",), mix=True)
                assert_selection(got, np.concatenate([ent, ent_h]), 10, what + ("mix",))


def test_narrow_mix_single_block(ce):
    """select_mix's one-block kernel (N, N_h <= 2048; the reduced set above is
    past it): C = 4, every dtype and view class, M below / at / above the batch."""
    from oracle import ce_oracle as O

    votes = np.random.default_rng(12).integers(-1, 4, (257, 30)).astype(np.int8)
    H = O.oracle_vote_table(votes)[0]
    ent_h = O.oracle_table_entropy(H)
    Hd = torch.from_numpy(H).cuda()
    for di, dt in enumerate(DTS):
        for vi, view in enumerate(VIEWS):
            M = (3, 4, 5, 9, 17)[(di + vi) % 5]
            layout = LAYOUTS[(di + vi) % 2]
            P, _, ent, _ = narrow_pool(50 + 5 * di + vi, dt, layout, view, 1608, M, 4)
            got = host_sel(ce.ops.select_mix(P, Hd, 10, layout))
            check_src(ce, P, layout, dt, (dt, view, M, layout, "mix"), mix=True)
            assert_selection(got, np.concatenate([ent, ent_h]), 10, (dt, view, M, layout, "mix"))


def test_zz_every_instantiation_ran(ce, capsys):
    """Over the whole module: both CommitteeSrc<dt, C, true> and <dt, C, false>
    were named by the library for every (dtype, C) with a vector instantiation,
    <dt, C, false> for the others, and every M of the list ran.  (Run alone, it
    first runs the single-block matrix it needs.)"""
    for dt in DTS:
        for view in VIEWS:
            if (dt, view) not in _SINGLE_DONE:
                run_single_block(ce, dt, view)
    want = {(dt, C, False) for dt in DTS for C in NARROW_C} | {(dt, C, True) for dt, C in HAS_VEC}
    assert SEEN_SRC == want, (sorted(want - SEEN_SRC), sorted(SEEN_SRC - want))
    assert SEEN_M >= set(NARROW_MS)
    with capsys.disabled():
        print("\nkernels named in this run (%d):" % len(SEEN_KERNELS))
        for k in sorted(SEEN_KERNELS):
            print("  " + (k or '""'))
        for dt in DTS:
            for kind in ("vec", "strided"):
                print("  wide sweep %s %s: %d class counts" % (dt, kind, sum(1 for d, _, k in SEEN_WIDE
                                                                               if d == dt and k == kind)))
        print("  CommitteeSrc seen: %s" % sorted(SEEN_SRC))
        print("  M seen: %s" % sorted(SEEN_M))


# ---------------------------------------------------------------------------
# 4. the error contract at the ends of the axes
# ---------------------------------------------------------------------------
# Asserted elsewhere and not repeated: a negative q, q = 0, a bad layout and a CPU tensor
# (test_gpu_parity.py::test_errors_are_loud); a bitmap on the strided wide stream
# (test_gpu_dispatch_pins.py; also test_wide_edges_deep_paths above); C > 2048 on the host alone
# (test_host.py::test_class_count_past_the_wide_limit_is_refused_without_gpu).
@pytest.mark.parametrize("dt", DTS)
def test_class_count_past_the_limit_raises(ce, dt):
    """C = 2049 (and C = 4095 / 2^17, whose summation plan would not fit its
    arrays): CEError CE_EUNSUPPORTED from committee_entropy and from select_mc at
    q = 10 / 65 / 2049, no kernel named, and a valid call right after is correct."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(3)
    N, M = 37, 2
    good_h = draw(rng, N * M * 9, dt)
    good = to_dev(good_h, dt).view(N, M, 9)
    ent = O.oracle_committee_entropy(good_h.reshape(N, M, 9), "NMC")
    for C in (2049, 4095, 1 << 17):
        P = to_dev(draw(rng, N * M * C, dt), dt).view(N, M, C)
        with pytest.raises(ce._lib.CEError) as ei:
            ce.ops.committee_entropy(P, "NMC")
        assert ei.value.code == ce._lib.CE_EUNSUPPORTED
        for q in (10, 65, 2049):
            with pytest.raises(ce._lib.CEError) as ei:
                ce.ops.select_mc(P, q, "NMC")
            assert ei.value.code == ce._lib.CE_EUNSUPPORTED and not isinstance(ei.value, ValueError)
            assert last_kernel(ce) == ""
        torch.cuda.synchronize()
        assert_bits(ce.ops.committee_entropy(good, "NMC").cpu().numpy(), ent, (dt, C, "after"))
        assert_selection(host_sel(ce.ops.select_mc(good, 10, "NMC")), ent, 10, (dt, C, "after"))


@pytest.mark.parametrize("C", [1, 5, 9, 16, 2048])
def test_wide_mean_output_is_refused(ce, C):
    """committee_entropy(return_mean=True) at a wide C: the 'mean output ... not
    implemented' error, for dense and strided rows, and the entropies alone still work."""
    from oracle import ce_oracle as O

    host = draw(np.random.default_rng(C), 9 * 2 * C * 2, "f32")
    for strides in ((2 * C, C, 1), (4 * C, 2 * C, 2)):
        P = to_dev(host, "f32").as_strided((9, 2, C), strides, 0)
        with pytest.raises(ce._lib.CEError, match="mean output .* not implemented") as ei:
            ce.ops.committee_entropy(P, "NMC", return_mean=True)
        assert ei.value.code == ce._lib.CE_EUNSUPPORTED
        ent = O.oracle_committee_entropy(hview(host, 0, (9, 2, C), strides), "NMC")
        assert_bits(ce.ops.committee_entropy(P, "NMC").cpu().numpy(), ent, (C, strides))


@pytest.mark.parametrize("dt", DTS)
def test_empty_pool(ce, dt):
    """N = 0: empty entropies and means; q slots of padding (NaN, -1) from
    select_mc at every q range, with a bitmap, batched and chunked -- for a
    narrow and a wide C, both layouts."""
    tdt = {"f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16}[dt]
    for C in (4, 9):
        for layout, shape in (("NMC", (0, 3, C)), ("MNC", (3, 0, C))):
            P = torch.empty(shape, dtype=tdt, device="cuda")
            assert ce.ops.committee_entropy(P, layout).shape == (0,)
            if C == 4:
                e, m = ce.ops.committee_entropy(P, layout, return_mean=True)
                assert e.shape == (0,) and m.shape == (0, C)
            for q in (1, 10, 65, 2049):
                v, i = host_sel(ce.ops.select_mc(P, q, layout))
                assert v.shape == i.shape == (q,) and np.isnan(v).all() and (i == -1).all(), (C, layout, q)
            v, i = host_sel(ce.ops.select_mc(P, 10, layout, excl=ce.ops.excl_bitmap(0, "cuda")))
            assert np.isnan(v).all() and (i == -1).all()
            v, i = host_sel(ce.ops.select_batched(P, torch.zeros(3, dtype=torch.int64, device="cuda"), 10, layout))
            assert v.shape == (2, 10) and np.isnan(v).all() and (i == -1).all()
            v, i = host_sel(ce.ops.MCChunkJob(10, layout).add(P).result())
            assert np.isnan(v).all() and (i == -1).all()
