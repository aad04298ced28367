"""Which kernel every selection entry point dispatches to, pinned.

tests/golden/dispatch_pins.json holds, per case, the ce_last_kernel() string
after each C-ABI call of the case, recorded on the MI355X by
tests/golden/gen_dispatch_pins.py.  The host layer must keep choosing the same
kernels (the strings name template arguments too), and every case's (vals, idx)
must equal the CPU oracle bit for bit.  ce_last_kernel() is empty on the
block-synchronous and single-block paths: there the results alone are checked.

The cases sit on both sides of every threshold the mc ladder tests: pools of
1 / 65 / 4096 / 4097 items (one block, the single-block kernels' limit), a bf16
pool of 5000 items (more than one block holds, fewer bytes than the small-pool
limit: blocks + a wave merge), 70000 items (the streaming kernels with the
merge folded in), q = 1 / 64 / 65 / 2048 / 2049 (streaming, block lists, sort),
and one shape per streaming kernel: item-major and member-major LDS-DMA tiles,
a strided view, C = 3, a contiguous wide committee, and a wide committee whose
rows are not 16-byte multiples (the kernel that neither folds nor takes a
bitmap)."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dispatch_pins.json")
QS = (1, 64, 65, 2048, 2049)


def _ce():
    import ce_amd
    import ce_amd.ops

    ce_amd.load()
    return ce_amd


def last_kernel():
    from ce_amd import _lib

    return _lib.load().ce_last_kernel().decode()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows(rng, shape, quant=16):
    """Coarse probabilities: exact entropy ties everywhere, so the lowest-position rule decides many places."""
    e = -np.log(rng.random(shape))
    return (np.floor(e / e.sum(-1, keepdims=True) * quant) / quant + 1e-3).astype(np.float32)


def _bf16(P32):
    """(device bf16 tensor, its uint16 bit patterns for the oracle)"""
    t = torch.from_numpy(P32).to(torch.bfloat16)
    return t.cuda(), t.view(torch.int16).numpy().view(np.uint16)


_POOLS = {}


def pool(name):
    """(device committee, layout, oracle entropies), built once per module run."""
    if name in _POOLS:
        return _POOLS[name]
    from oracle import ce_oracle as O

    rng = np.random.default_rng(sum(map(ord, name)))
    kind, n = name.rsplit("_", 1)
    N = int(n)
    if kind == "f32":  # item-major f32, M = 4, C = 4 (64-byte items: the direct kernel)
        P = _rows(rng, (N, 4, 4))
        out = dev(P), "NMC", O.oracle_committee_entropy(P, "NMC")
    elif kind == "bf16":
        P = _rows(rng, (N, 4, 4))
        d, bits = _bf16(P)
        out = d, "NMC", O.oracle_committee_entropy(bits, "NMC")
    elif kind == "nmc16":  # item-major, M = 16: 256-byte items, the LDS-DMA tiles
        P = _rows(rng, (N, 16, 4))
        out = dev(P), "NMC", O.oracle_committee_entropy(P, "NMC")
    elif kind == "mnc4":  # the reference's member-major stack
        P = _rows(rng, (4, N, 4))
        out = dev(P), "MNC", O.oracle_committee_entropy(P, "MNC")
    elif kind == "strided":  # every second class of a wider tensor: no vector loads, no tiles
        P = _rows(rng, (N, 4, 8))
        out = dev(P)[:, :, ::2], "NMC", O.oracle_committee_entropy(P[:, :, ::2], "NMC")
    elif kind == "c3":
        P = _rows(rng, (N, 4, 3))
        out = dev(P), "NMC", O.oracle_committee_entropy(P, "NMC")
    elif kind in ("wide100", "wide104"):  # contiguous bf16 rows of 200 / 208 bytes (208: 16-byte multiples, vector loads)
        P = _rows(rng, (N, 2, int(kind[4:])), quant=64)
        d, bits = _bf16(P)
        out = d, "NMC", O.oracle_committee_entropy(bits, "NMC")
    elif kind == "wide129":  # 516-byte rows: the strided wide kernel
        P = _rows(rng, (N, 2, 129), quant=64)
        out = dev(P), "NMC", O.oracle_committee_entropy(P, "NMC")
    else:
        raise KeyError(name)
    _POOLS[name] = out
    return out


def expect(ent, q, keep=None, base=0):
    """(vals, idx) of the oracle's total order, q slots."""
    from oracle import ce_oracle as O

    if keep is not None:
        order = keep[O.canonical_order(ent[keep], q)]
    else:
        order = O.canonical_order(ent, q)
    return ent[order], order + base


def check(got, want):
    (v, i), (ev, ei) = got, want
    v, i = v.cpu().numpy().reshape(-1), i.cpu().numpy().reshape(-1)
    n = len(ei)
    assert np.array_equal(i[:n], ei) and (i[n:] == -1).all()
    assert np.array_equal(v[:n].view(np.uint64), np.ascontiguousarray(ev).view(np.uint64))  # bit for bit
    assert np.isnan(v[n:]).all()


# ---- the cases: name -> function returning the list of ce_last_kernel() strings
def _bitmap(ce, N):
    ex = ce.ops.excl_bitmap(N, "cuda")
    ce.ops.mark_selected(ex, N, torch.arange(0, N, 3, device="cuda"))
    return ex, np.flatnonzero(np.arange(N) % 3 != 0)


def c_select_mc(name, q, excl=False):
    def run(ce):
        P, lay, ent = pool(name)
        ex, keep = _bitmap(ce, len(ent)) if excl else (None, None)
        try:
            got = ce.ops.select_mc(P, q, lay, base_idx=7, excl=ex)
        except ce._lib.CEError as e:  # the strided wide kernel takes no bitmap, and a wide C has no other
            assert excl and name.startswith("wide") and q <= 64, e
            return ["unsupported: " + last_kernel()]
        k = last_kernel()
        check(got, expect(ent, q, keep, 7))
        return [k]
    return run


def c_cands(name, q):
    def run(ce):
        P, lay, ent = pool(name)
        rec = ce.ops.MCPlan(P, q, lay, base_idx=3).step_cands()
        k = last_kernel()
        check(ce.ops.merge_cands(rec, q), expect(ent, q, None, 3))
        return [k]
    return run


def c_two_stage(name, q):
    def run(ce):
        P, lay, ent = pool(name)
        plan = ce.ops.MCPlan(P, q, lay)
        plan.partial()
        ks = [last_kernel()]
        v, i = plan.finish()
        check((v.clone(), i.clone()), expect(ent, q))
        plan.partial()
        ks.append(last_kernel())
        check(ce.ops.merge_cands(plan.finish_cands(), q), expect(ent, q))
        return ks
    return run


def c_chunks(name, q):
    def run(ce):
        P, lay, ent = pool(name)
        N = len(ent)
        cut = N // 2 + 1
        job = ce.ops.MCChunkJob(q, lay)
        ks = []
        for lo, hi in ((0, cut), (cut, N)):
            job.add(P[lo:hi] if lay == "NMC" else P[:, lo:hi])
            ks.append(last_kernel())
        check(job.result(), expect(ent, q))
        return ks
    return run


def c_mix(N, Nh, q):
    def run(ce):
        from oracle import ce_oracle as O

        P, lay, ent = pool(f"f32_{N}")
        votes = np.random.default_rng(Nh).integers(-1, 4, (Nh, 30)).astype(np.int8)
        H = O.oracle_vote_table(votes)[0]
        got = ce.ops.select_mix(P, dev(H), q, lay)
        k = last_kernel()
        check(got, expect(np.concatenate([ent, O.oracle_table_entropy(H)]), q))
        return [k]
    return run


def c_batched(sizes, q):
    def run(ce):
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        P, lay, ent = pool(f"f32_{int(offs[-1])}")
        v, i = ce.ops.select_batched(P, dev(offs), q, lay)
        k = last_kernel()
        for u in range(len(sizes)):
            check((v[u], i[u]), expect(ent[offs[u]:offs[u + 1]], q))
        return [k]
    return run


def c_frames(q):
    def run(ce):
        from oracle import ce_oracle as O

        rng = np.random.default_rng(40 + q)
        N, C = 900, 4
        counts = rng.integers(1, 40, N)
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        s_id = np.repeat(np.arange(N), counts)
        members = [_rows(rng, (int(offs[-1]), C), 8).astype(dt) for dt in (np.float64, np.float32)]
        song = _rows(rng, (N, C), 4)
        P = np.array([O.ref_group_mean(m, s_id)[0] for m in members] + [song])
        got = ce.ops.select_frames([dev(m) for m in members] + [dev(song)], dev(offs), q)
        k = last_kernel()
        check(got, expect(O.oracle_committee_entropy(P, "MNC"), q))
        return [k]
    return run


def c_topq(N, q):
    def run(ce):
        _, _, ent = pool(f"f32_{N}")
        got = ce.ops.topq(dev(ent), q, base_idx=5)
        k = last_kernel()
        check(got, expect(ent, q, None, 5))
        return [k]
    return run


def _cases():
    c = {}
    for N in (1, 65, 4096, 4097):
        for q in QS:
            c[f"select_mc-f32_{N}-q{q}"] = c_select_mc(f"f32_{N}", q)
            c[f"topq-{N}-q{q}"] = c_topq(N, q)
        for q in (1, 65, 2049):
            c[f"select_mc_excl-f32_{N}-q{q}"] = c_select_mc(f"f32_{N}", q, excl=True)
            c[f"cands-f32_{N}-q{q}"] = c_cands(f"f32_{N}", q)
        for q in (1, 65):
            c[f"two_stage-f32_{N}-q{q}"] = c_two_stage(f"f32_{N}", q)
    big = ("bf16_5000", "nmc16_70000", "mnc4_70000", "strided_70000", "c3_70000", "wide100_5000", "wide104_5000",
           "wide129_5000")
    for name in big:
        for q in QS:
            c[f"select_mc-{name}-q{q}"] = c_select_mc(name, q)
        for q in (64, 65, 2049):
            c[f"cands-{name}-q{q}"] = c_cands(name, q)
        for q in (64, 65, 2048):
            c[f"two_stage-{name}-q{q}"] = c_two_stage(name, q)
        for q in (10, 65, 2049):
            c[f"chunks-{name}-q{q}"] = c_chunks(name, q)
    for name in ("nmc16_70000", "wide104_5000", "wide129_5000"):
        for q in (1, 65, 2049):
            c[f"select_mc_excl-{name}-q{q}"] = c_select_mc(name, q, excl=True)
    for q in (10, 65, 2049):
        c[f"chunks-f32_4097-q{q}"] = c_chunks("f32_4097", q)
    for N, Nh in ((4096, 800), (4097, 800), (65, 5000)):
        for q in (1, 64, 65, 2049):
            c[f"mix-{N}-{Nh}-q{q}"] = c_mix(N, Nh, q)
    for sizes in ((700, 800, 1500), (30000, 0, 40000)):
        for q in (10, 64, 65, 2049):
            c[f"batched-{sum(sizes)}-q{q}"] = c_batched(sizes, q)
    for q in (10, 65):
        c[f"frames-q{q}"] = c_frames(q)
    return c


CASES = _cases()


@pytest.fixture(scope="module")
def ce():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return _ce()


@pytest.fixture(scope="module")
def pins():
    with open(PINS) as f:
        return {case: g["kernels"] for g in json.load(f)["groups"] for case in g["cases"]}


def test_dispatch_pins(ce, pins):
    """Every case: the oracle's (vals, idx) bit for bit (checked inside the
    case) and the kernels the recorded commit dispatched to."""
    assert sorted(pins) == sorted(CASES)
    wrong = {}
    for name, run in CASES.items():
        got = run(ce)
        if got != pins[name]:
            wrong[name] = (got, pins[name])
    assert not wrong, wrong
