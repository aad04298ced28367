"""Generator of abi_host_pins.json: what the C-ABI's host layer answers without
a GPU.  Run it against a build of the commit whose behaviour is to be pinned
(python tests/golden/gen_abi_host_pins.py [path/to/libce_amd.so]); the test
tests/test_host_pins.py replays both tables against the tree's library.

Table "sizes": every ce_*_workspace_bytes function over a grid of N, q, U, N_h
(negative and zero arguments included).
Table "calls": return code and ce_last_error() text of calls that the library
answers before any HIP call: every invalid-argument class, a workspace one byte
short, q = 0, q > CE_MAX_Q on the two-stage API, misaligned records, and calls
with two faults at once (they pin the order of the checks).  No call here may
reach a launch: each must fail, or be a q = 0 call returning CE_OK.
"""
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "abi_host_pins.json")

NS = [-1, 0, 1, 63, 64, 65, 4096, 4097, 65536, 65537, 10**8, 2**32]
QS = [-1, 0, 1, 64, 65, 2048, 2049, 100000]
US = [0, 1, 64, 500]
NHS = [0, 1, 1300, 5000]

SIZE_GRIDS = {
    "ce_topq_workspace_bytes": list(itertools.product(NS, QS)),
    "ce_select_mc_workspace_bytes": list(itertools.product(NS, QS)),
    "ce_select_mc_chunk_workspace_bytes": list(itertools.product(NS, QS)),
    "ce_select_frames_workspace_bytes": list(itertools.product(NS, QS)),
    "ce_select_mix_workspace_bytes": list(itertools.product(NS, NHS, QS)),
    "ce_select_batched_workspace_bytes": list(itertools.product(NS, US, QS)),
}

P, P2, Q = 0x10000, 0x20000, 0x30000  # never dereferenced: fake device pointers (16-byte aligned)
ODD = 0x10008                         # a pointer that is not 16-byte aligned
HUGE = 1 << 62                        # a workspace size no formula exceeds


class _Member(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("dtype", ctypes.c_int32), ("song_level", ctypes.c_int32),
                ("ld", ctypes.c_int64)]


def load(path=None):
    for p in (ROOT, os.path.join(ROOT, "consensus-entropy_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from ce_amd import _lib

    if path is None:
        return _lib.load()
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


def invoke(lib, fn, args):
    """(rc, ce_last_error()) of one call; {"members": [[p, dtype, song_level, ld], ...]}
    stands for a host array of ce_member."""
    keep, real = [], []
    for a in args:
        if isinstance(a, dict):
            arr = (_Member * max(len(a["members"]), 1))()
            for i, m in enumerate(a["members"]):
                arr[i] = _Member(*m)
            keep.append(arr)
            a = ctypes.cast(arr, ctypes.c_void_p)
        real.append(a)
    rc = getattr(lib, fn)(*real)
    return int(rc), lib.ce_last_error().decode()


def size_rows(lib):
    """fn -> its values over SIZE_GRIDS[fn], in the grid's order"""
    return {fn: [int(getattr(lib, fn)(*a)) for a in grid] for fn, grid in SIZE_GRIDS.items()}


def call_list(lib):
    """[fn, args, q0] -- q0: a q = 0 call (the only calls that may return CE_OK)."""
    mcws = lambda n, q: int(lib.ce_select_mc_workspace_bytes(n, q))
    calls = []

    def add(fn, *args, q0=False):
        calls.append([fn, list(args), q0])

    # ---- ce_select_mc / _excl / _cands: (p, dt, N, M, C, sN, sM, sC) ...
    def comm(p=P, dt=0, N=1000, M=4, C=4, sN=16, sM=4, sC=1):
        return [p, dt, N, M, C, sN, sM, sC]

    bad_comms = [comm(p=None), comm(N=-1), comm(M=0), comm(C=0), comm(dt=3), comm(dt=-1), comm(p=None, M=0)]

    def mc(c=None, q=10, base=0, ws=P2, wsb=None, val=Q, idx=Q, excl="no"):
        c = c or comm()
        wsb = mcws(c[2], q) if wsb is None else wsb
        if excl == "no":
            add("ce_select_mc", *c, q, base, ws, wsb, val, idx, None, q0=(q == 0))
        else:
            add("ce_select_mc_excl", *c, excl, q, base, ws, wsb, val, idx, None,
                q0=(q == 0))

    for c in bad_comms:
        mc(c)
        mc(c, q=-1)        # two faults: the committee is checked first
        mc(c, wsb=8)
    mc(q=-1)
    mc(q=-1, val=None)     # q before the outputs
    mc(q=-1, ws=None)
    mc(val=None)
    mc(idx=None)
    mc(val=None, wsb=8)    # outputs before the workspace
    mc(ws=None)
    mc(wsb=mcws(1000, 10) - 1)
    mc(q=65, wsb=mcws(1000, 65) - 1)
    mc(q=3000, wsb=mcws(1000, 3000) - 1)
    mc(q=0)
    mc(q=0, val=None, idx=None)
    mc(q=0, ws=None)       # the workspace contract holds before q = 0 returns
    mc(q=0, wsb=mcws(1000, 0) - 1)
    mc(comm(N=0, p=None), q=0)
    mc(comm(N=2**32), q=3000, wsb=HUGE)  # the sort path's record limit
    mc(excl=None)
    mc(comm(M=0), excl=None)             # the bitmap is checked before the committee
    mc(q=-1, excl=None)
    mc(comm(N=0), q=-1, excl=None)
    mc(excl=P, q=-1)
    mc(excl=P, val=None)
    mc(excl=P, ws=None)
    mc(excl=P, q=0)
    mc(excl=P, q=0, ws=None)

    def cands(c=None, q=10, base=0, ws=P2, wsb=None, out=Q):
        c = c or comm()
        wsb = mcws(c[2], q) if wsb is None else wsb
        add("ce_select_mc_cands", *c, q, base, ws, wsb, out, None, q0=(q == 0))

    for c in bad_comms:
        cands(c)
        cands(c, out=ODD)
    cands(q=-1)
    cands(q=-1, out=None)
    cands(out=None)
    cands(out=ODD)
    cands(out=ODD, ws=None)
    cands(ws=None)
    cands(wsb=mcws(1000, 10) - 1)
    cands(q=3000, wsb=mcws(1000, 3000) - 1)
    cands(q=0)
    cands(q=0, out=None)
    cands(q=0, out=ODD)
    cands(q=0, ws=None)
    cands(comm(N=2**32), q=3000, wsb=HUGE)

    # ---- the two-stage API
    def lists_bytes(n, q):  # the partial / finish contract: the lists alone
        g = min(max((n + 63) // 64, 1), 1024)
        return 65536 + g * q * 16 + 256

    def partial(c=None, q=10, ws=P2, wsb=HUGE):
        add("ce_select_mc_partial", *(c or comm()), q, 0, ws, wsb, None, q0=(q == 0))

    partial(q=2049)
    partial(comm(M=0), q=2049)           # the refusal comes first
    partial(q=100000, ws=None)
    partial(q=0)
    partial(comm(p=None, M=0), q=0, ws=None)
    partial(q=-1)
    partial(comm(M=0), q=-1)             # q <= 0 is answered before the committee is looked at
    for c in bad_comms:
        partial(c)
        partial(c, ws=None)
    partial(ws=None)
    partial(wsb=lists_bytes(1000, 10) - 1)
    partial(q=65, wsb=lists_bytes(1000, 65) - 1)

    def finish(N=1000, q=10, ws=P2, wsb=HUGE, val=Q, idx=Q):
        add("ce_select_finish", N, q, ws, wsb, val, idx, None, q0=(q == 0))

    finish(q=-1)
    finish(q=-1, N=-1)
    finish(q=2049)
    finish(q=2049, N=-1)
    finish(q=0)
    finish(q=0, N=-1, ws=None, val=None)
    finish(N=-1)
    finish(val=None)
    finish(idx=None)
    finish(N=-1, ws=None)
    finish(ws=None)
    finish(wsb=lists_bytes(1000, 10) - 1)
    finish(N=10**8, q=2048, wsb=lists_bytes(10**8, 2048) - 1)

    def finish_cands(N=1000, q=10, ws=P2, wsb=HUGE, out=Q):
        add("ce_select_finish_cands", N, q, ws, wsb, out, None, q0=(q == 0))

    finish_cands(q=-1)
    finish_cands(q=2049)
    finish_cands(q=2049, out=ODD)
    finish_cands(q=0)
    finish_cands(q=0, out=ODD, ws=None)
    finish_cands(N=-1)
    finish_cands(out=None)
    finish_cands(out=ODD)
    finish_cands(N=-1, out=ODD)
    finish_cands(out=ODD, ws=None)
    finish_cands(ws=None)
    finish_cands(wsb=lists_bytes(1000, 10) - 1)

    def merge_cands(c=P, nl=3, q=10, val=Q, idx=Q):
        add("ce_merge_cands", c, nl, q, val, idx, None, q0=(q == 0))

    merge_cands(q=-1)
    merge_cands(q=0)
    merge_cands(q=0, c=None, nl=0)
    merge_cands(nl=0)
    merge_cands(c=None)
    merge_cands(val=None)
    merge_cands(idx=None)
    merge_cands(c=ODD)
    merge_cands(c=ODD, nl=0)
    merge_cands(c=ODD, q=3000)

    # ---- chunked pools
    chws = lambda n, q: int(lib.ce_select_mc_chunk_workspace_bytes(n, q))

    def chunk(c=None, q=10, base=0, run=Q, first=1, ws=P2, wsb=None):
        c = c or comm()
        wsb = chws(c[2], q) if wsb is None else wsb
        add("ce_select_mc_chunk", *c, q, base, run, first, ws, wsb, None, q0=(q == 0))

    chunk(q=-1)
    chunk(q=-1, run=None)
    chunk(q=0)
    chunk(comm(p=None, M=0), q=0, run=None, ws=None, wsb=0)  # q = 0 returns before everything else
    chunk(run=None)
    chunk(run=ODD)
    chunk(run=ODD, first=0)
    chunk(comm(N=-1), run=None)
    chunk(comm(N=-1))
    chunk(base=-1)
    chunk(comm(N=-1), ws=None)
    chunk(ws=None)
    chunk(wsb=chws(1000, 10) - 1)
    chunk(wsb=chws(1000, 10) - 1, first=0)
    chunk(q=65, wsb=chws(1000, 65) - 1)
    chunk(q=3000, wsb=chws(1000, 3000) - 1)
    chunk(comm(M=0), wsb=8)              # the workspace before the committee
    for c in (comm(p=None), comm(M=0), comm(C=0), comm(dt=3)):
        chunk(c, wsb=HUGE)
        chunk(c, q=3000, wsb=HUGE, first=0)
    chunk(comm(N=2**32), q=3000, wsb=HUGE)
    chunk(comm(N=2**32), q=3000, wsb=HUGE, first=0)

    # ---- top-q of an entropy vector
    tqws = lambda n, q: int(lib.ce_topq_workspace_bytes(n, q))

    def topq(ent=P, N=1000, q=10, base=0, ws=P2, wsb=None, val=Q, idx=Q):
        wsb = tqws(N, q) if wsb is None else wsb
        add("ce_topq", ent, N, q, base, ws, wsb, val, idx, None, q0=(q == 0))

    topq(q=-1)
    topq(q=-1, N=-1)
    topq(N=-1)
    topq(q=0, N=-1)                      # the arguments are checked before q = 0 returns
    topq(q=0, ent=None)
    topq(val=None)
    topq(idx=None)
    topq(ent=None)
    topq(ent=None, ws=None)
    topq(q=0)
    topq(q=0, ws=None, wsb=0, val=None, idx=None)  # ... but not the workspace
    topq(ws=None)
    topq(wsb=tqws(1000, 10) - 1)
    topq(q=2048, wsb=tqws(1000, 2048) - 1)
    topq(q=2049, wsb=tqws(1000, 2049) - 1)
    topq(N=2**32, q=3000, wsb=HUGE)

    def topq_merge(vals=P, idx=P2, nl=3, q=10, oval=Q, oidx=Q):
        add("ce_topq_merge", vals, idx, nl, q, oval, oidx, None, q0=(q == 0))

    topq_merge(q=-1)
    topq_merge(q=0)
    topq_merge(q=0, vals=None, nl=0)
    topq_merge(nl=0)
    topq_merge(vals=None)
    topq_merge(idx=None)
    topq_merge(oval=None)
    topq_merge(oidx=None, q=3000)

    # ---- the mix
    mxws = lambda n, nh, q: int(lib.ce_select_mix_workspace_bytes(n, nh, q))

    def mix(c=None, hc=P, Nh=1300, ld=4, q=10, ws=P2, wsb=None, val=Q, idx=Q):
        c = c or comm()
        wsb = mxws(c[2], Nh, q) if wsb is None else wsb
        add("ce_select_mix", *c, hc, Nh, ld, q, ws, wsb, val, idx, None,
            q0=(q == 0))

    for c in bad_comms:
        mix(c)
        mix(c, Nh=-1)
    mix(q=-1)
    mix(q=-1, Nh=-1)
    mix(Nh=-1)
    mix(hc=None)
    mix(ld=3)
    mix(val=None)
    mix(idx=None)
    mix(Nh=-1, ws=None)
    mix(val=None, wsb=8)
    mix(ws=None)
    mix(wsb=mxws(1000, 1300, 10) - 1)
    mix(q=3000, wsb=mxws(1000, 1300, 3000) - 1)
    mix(q=0)
    mix(q=0, val=None, idx=None, hc=None, Nh=0)
    mix(q=0, ws=None)
    mix(q=0, Nh=-1)
    mix(comm(N=2**31), Nh=2**31, q=3000, wsb=HUGE)

    # ---- batched users
    btws = lambda n, u, q: int(lib.ce_select_batched_workspace_bytes(n, u, q))

    def batched(c=None, off=P, U=3, q=10, ws=P2, wsb=None, val=Q, idx=Q):
        c = c or comm()
        wsb = btws(c[2], U, q) if wsb is None else wsb
        add("ce_select_batched", *c, off, U, q, ws, wsb, val, idx, None,
            q0=(q == 0))

    for c in bad_comms:
        batched(c)
        batched(c, U=0)
    batched(q=-1)
    batched(q=-1, U=0)
    batched(U=0)
    batched(U=-1, ws=None)
    batched(off=None)
    batched(val=None)
    batched(idx=None)
    batched(val=None, wsb=8)
    batched(ws=None)
    batched(wsb=btws(1000, 3, 10) - 1)
    batched(U=500, wsb=btws(1000, 500, 10) - 1)
    batched(q=3000, wsb=btws(1000, 3, 3000) - 1)
    batched(q=0)
    batched(q=0, val=None, idx=None)
    batched(q=0, ws=None)
    batched(q=0, U=0)
    batched(q=3000, U=1 << 23, wsb=HUGE)
    batched(comm(N=1 << 40), q=3000, wsb=HUGE)
    batched(comm(N=1 << 40), q=3000, U=1 << 23, wsb=HUGE)  # the users are counted first
    batched(comm(N=2**32), q=3000, wsb=HUGE)

    # ---- frames: (members, M, C, offsets, perm, N, q, base_idx, ws, ws_bytes, val, idx, stream)
    frws = lambda n, q: int(lib.ce_select_frames_workspace_bytes(n, q))
    good = [[P, 0, 0, 4], [P2, 1, 1, 8]]

    def frames(mem=good, M=None, C=4, off=P, N=1000, q=10, ws=P2, wsb=None, val=Q, idx=Q):
        wsb = frws(N, q) if wsb is None else wsb
        M = len(mem) if M is None else M
        add("ce_select_frames", {"members": mem} if mem is not None else None, M, C, off, None, N, q, 0, ws, wsb, val,
            idx, None, q0=(q == 0))

    frames(q=-1)
    frames(q=-1, mem=None, M=2)
    frames(mem=None, M=2)
    frames(M=0)
    frames(M=10**6)
    frames(M=0, N=-1)
    frames(N=-1)
    frames(off=None)
    frames(val=None)
    frames(idx=None)
    frames(N=-1, C=5)
    frames(C=5)
    frames(C=1, ws=None)                 # the class count before the workspace
    frames(ws=None)
    frames(wsb=frws(1000, 10) - 1)
    frames(q=65, wsb=frws(1000, 65) - 1)
    frames(q=2049, wsb=frws(1000, 2049) - 1)
    frames(mem=[[P, 2, 0, 4]])           # a bf16 member
    frames(mem=[[P, 2, 0, 4]], ws=None)  # the workspace before the members
    frames(mem=[[P, 0, 0, 4], [None, 0, 0, 4]])
    frames(mem=[[P, 0, 0, 3]])
    frames(mem=[[None, 2, 0, 3]])
    frames(q=0)
    frames(q=0, val=None, idx=None)
    frames(q=0, ws=None)
    frames(q=0, C=5)
    frames(q=0, mem=[[P, 0, 0, 3]])
    return calls


def call_rows(lib):
    rows = []
    for fn, args, q0 in call_list(lib):
        rc, err = invoke(lib, fn, args)
        assert rc != 0 or q0, f"{fn}{args}: rc={rc} {err!r} (a pinned call must fail or be a q = 0 call)"
        rows.append({"fn": fn, "args": args, "rc": rc, "error": err if rc else ""})
    return rows


def main():
    lib = load(sys.argv[1] if len(sys.argv) > 1 else None)
    sizes, calls = size_rows(lib), call_rows(lib)
    with open(OUT, "w") as f:  # one line per function / per call
        f.write('{"version": %s,\n "grid": %s,\n "sizes": {\n' % (
            json.dumps(lib.ce_version().decode()), json.dumps({"N": NS, "q": QS, "U": US, "N_h": NHS})))
        f.write(",\n".join("  %s: %s" % (json.dumps(fn), json.dumps(v, separators=(",", ":"))) for fn, v in sizes.items()))
        f.write('\n },\n "calls": [\n')
        f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in calls))
        f.write("\n ]}\n")
    print(OUT, sum(len(v) for v in sizes.values()), "sizes,", len(calls), "calls")


if __name__ == "__main__":
    main()
