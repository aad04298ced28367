"""CPU checks of the C-ABI's host layer: every workspace size and every
answer the library gives before its first HIP call equal the pinned ones
(tests/golden/abi_host_pins.json, written by tests/golden/gen_abi_host_pins.py
at the commit before the host layer moved to one workspace layout), and the
layout itself (csrc/ce_ws.hpp) is sound under ASan + UBSan."""
import importlib.util
import json
import os
import subprocess

from conftest import GOLDEN, PKG_DIR


def _gen():
    spec = importlib.util.spec_from_file_location("gen_abi_host_pins", os.path.join(GOLDEN, "gen_abi_host_pins.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _pins():
    with open(os.path.join(GOLDEN, "abi_host_pins.json")) as f:
        return json.load(f)


def test_workspace_sizes_are_the_pinned_ones():
    gen, pins = _gen(), _pins()
    lib = gen.load()
    assert pins["grid"] == {"N": gen.NS, "q": gen.QS, "U": gen.US, "N_h": gen.NHS}  # the grid the values are over
    got = gen.size_rows(lib)
    assert sorted(pins["sizes"]) == sorted(got) and all(len(pins["sizes"][fn]) == len(got[fn]) for fn in got)
    wrong = [(fn, a, g, w) for fn in got for a, g, w in zip(gen.SIZE_GRIDS[fn], got[fn], pins["sizes"][fn]) if g != w]
    assert not wrong, wrong[:10]


def test_host_answers_are_the_pinned_ones():
    """Return code and ce_last_error() text of every pinned call (none reaches a launch)."""
    gen, pins = _gen(), _pins()
    lib = gen.load()
    assert len(pins["calls"]) >= 250
    assert {c["fn"] for c in pins["calls"]} >= {
        "ce_select_mc", "ce_select_mc_excl", "ce_select_mc_cands", "ce_select_mc_partial", "ce_select_finish",
        "ce_select_finish_cands", "ce_merge_cands", "ce_select_mc_chunk", "ce_topq", "ce_topq_merge", "ce_select_mix",
        "ce_select_batched", "ce_select_frames"}
    wrong = []
    for c in pins["calls"]:
        rc, err = gen.invoke(lib, c["fn"], c["args"])
        if rc != c["rc"] or (rc and err != c["error"]):
            wrong.append((c["fn"], c["args"], (rc, err), (c["rc"], c["error"])))
    assert not wrong, wrong[:10]


def test_workspace_layout_under_sanitizers():
    """make sanitize-ws: csrc/ce_ws_sanitize.cpp (ce_ws.hpp alone, host compiler, ASan + UBSan)."""
    r = subprocess.run(["make", "-C", PKG_DIR, "sanitize-ws"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "layouts" in r.stdout and ": ok" in r.stdout
