"""IPCR_JIT_INVMASK (jit.cpp): the specialised filter's inv-plane loads of its own block are raw buffer loads that a clean
column's lane sends out of range.  Checked in the gfx950 ISA of the C2 and C3 kernels, against the knob-0 form: no
waterfall around them, and the main loop keeps its prefetch depth (its vmcnt waits are no lower).  Needs hipcc only."""
import os
import re
import subprocess

import pytest

HIPCC = "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


def emit(name, knob, tmp):
    from ipcr_amd import engine
    from ipcr_amd.workloads import c2_pairs, c3_pairs
    if name == "c2":
        cfg, pairs = engine.Config(MaxMM=2, TerminalWindow=5, MaxLen=2000, HitCap=10000, SeedLen=12), c2_pairs()
    else:
        cfg, pairs = engine.Config(MaxMM=3, TerminalWindow=3, MaxLen=2000, HitCap=10000, SeedLen=12, Circular=True), c3_pairs()
    old = os.environ.get("IPCR_JIT_INVMASK")
    os.environ["IPCR_JIT_INVMASK"] = knob
    try:
        cp = engine.New(cfg).CompilePanel(pairs)
        src = cp.filter_source(0)
        cp.close()
    finally:
        if old is None:
            del os.environ["IPCR_JIT_INVMASK"]
        else:
            os.environ["IPCR_JIT_INVMASK"] = old
    assert src
    path = os.path.join(tmp, "%s_%s.hip" % (name, knob))
    with open(path, "w") as f:
        f.write(src)
    asm = subprocess.check_output([HIPCC, "--offload-arch=gfx950", "-O3", "-S", "--cuda-device-only", "-o", "-", path],
                                  stderr=subprocess.DEVNULL).decode()
    return src, asm.splitlines()


def main_loop(lines):
    """the instructions of the main loop: from its header label to the branch back to it"""
    for i, ln in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):\s*; =>This Loop Header: Depth=1", ln)
        if m:
            for j in range(i + 1, len(lines)):
                if re.search(r"s_cbranch_\w+\s+" + re.escape(m.group(1)) + r"$", lines[j].strip()):
                    return lines[i:j + 1]
    raise AssertionError("main loop not found")


def vmcnts(lines):
    return sorted(int(x) for ln in lines for x in re.findall(r"vmcnt\((\d+)\)", ln))


@pytest.mark.parametrize("name", ["c2", "c3"])
def test_inv_loads_are_buffer_loads(name, tmp_path):
    src_on, on = emit(name, "1", str(tmp_path))
    src_off, off = emit(name, "0", str(tmp_path))
    assert "raw_buffer_load_b128" in src_on and "raw_buffer_load_b128" not in src_off
    loop_on, loop_off = main_loop(on), main_loop(off)
    buf = [ln for ln in loop_on if "buffer_load_dwordx4" in ln]
    glob = sum("global_load_dwordx4" in ln for ln in loop_off)
    # one inv load per quad of the loop, non-temporal as the lo / hi loads; the lo / hi loads stay global loads
    assert buf and all(" nt" in ln for ln in buf), buf
    assert len(buf) + sum("global_load_dwordx4" in ln for ln in loop_on) == glob
    assert not any("buffer_load" in ln for ln in off)
    # no waterfall: the buffer loads add no exec-mask loop (the kernel's own branches are the same in both forms) and
    # the descriptor is read into SGPRs once, not per load
    assert sum("s_and_saveexec" in ln for ln in on) == sum("s_and_saveexec" in ln for ln in off)
    assert not any("v_readfirstlane" in ln for ln in loop_on)
    # the prefetch depth holds: the loop's waits let as many loads stay in flight as without the mask
    w_on, w_off = vmcnts(loop_on), vmcnts(loop_off)
    assert w_on and w_off and w_on[0] >= w_off[0], (w_on, w_off)
