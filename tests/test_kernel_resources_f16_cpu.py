"""test_kernel_resources_cpu's two checks for the one-term tower kernels
(AZ_CONV_F16: tower16h_kernel, tower16h_dual_kernel): no spilled VGPR in the
double-buffered, input-row and dual forms, the in-place fallbacks and the
192-row tile within the three-term kernels' bounds (<= 8, <= 24); and, in
the compiled ISA, nothing of the compiler's between a one-term group's loads
and the next group or the drain -- no vmcnt wait, no scratch access, no
instruction touching a register still in flight.  The ISA walk is
test_kloop_asm_invariants' own, applied to the new names."""
import os
import re
import subprocess

import pytest

import test_kernel_resources_cpu as base

CSRC, HIPCC = base.CSRC, base.HIPCC
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@needs_hipcc
def test_one_term_kernel_register_budget(tmp_path):
    out = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
         "--cuda-device-only", "-c", os.path.join(CSRC, "az_tower16.hip"), "-o", str(tmp_path / "t.o")],
        capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    spills, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and name:
            spills[name] = int(m.group(1))
    h = {k: v for k, v in spills.items() if "tower16h_" in k}
    assert len(h) == 10, sorted(spills)  # a twin of each of the 9 tower16_kernel forms and of the dual launch

    def form(tag):
        got = [v for k, v in h.items() if tag in k]
        assert len(got) == 1, (tag, sorted(h))
        return got[0]
    # <tile blocks, wave groups, input-row form (chess), double-buffered>
    for tag in ("tower16h_kernelILi8ELi2ELb0ELb1E", "tower16h_kernelILi6ELi2ELb0ELb1E", "tower16h_kernelILi8ELi2ELb1ELb1E",
                "tower16h_kernelILi4ELi2ELb1ELb1E", "tower16h_dual_kernelILi8ELi6ELb1E"):
        assert form(tag) == 0, h
    inplace = [v for k, v in h.items() if "tower16h_kernel" in k and "Lb0EEEv" in k and "ILi12E" not in k]
    assert len(inplace) == 4 and max(inplace) <= 8, h
    assert form("tower16h_kernelILi12ELi2ELb0ELb0E") <= 24, h


@needs_hipcc
def test_one_term_kloop_asm_invariants(tmp_path):
    s_file = tmp_path / "t.s"
    out = subprocess.run(
        [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-S",
         os.path.join(CSRC, "az_tower16.hip"), "-o", str(s_file)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = s_file.read_text().split("\n")
    starts = [i for i, l in enumerate(lines)
              if re.match(r"^_ZN2az12_GLOBAL__N_1(15tower16h_kernel|20tower16h_dual_kernel)\S*:", l)]
    assert len(starts) == 10
    groups_seen = 0
    for st in starts:
        groups_seen += check_function(lines, st)
    assert groups_seen > 0


def check_function(lines, st):
    """One kernel's walk (test_kloop_asm_invariants' body): the groups it saw."""
    _regs = base._regs
    en = next(i for i in range(st, len(lines)) if lines[i].startswith(".Lfunc_end"))
    blocks, names, cur, kind, seg = [], {}, [], "gap", []
    for l in lines[st + 1:en]:
        m = re.match(r"^(\.LBB\S+):", l)
        if m:
            cur.append((kind, seg))
            blocks.append(cur)
            names[m.group(1)] = len(blocks)
            cur, kind, seg = [], "gap", []
            continue
        if ";;#ASMSTART" in l or ";;#ASMEND" in l:
            cur.append((kind, seg))
            seg, kind = [], ("asm" if ";;#ASMSTART" in l else "gap")
            continue
        code = l.split(";")[0].strip()
        if code and not code.startswith("."):
            seg.append(code)
    cur.append((kind, seg))
    blocks.append(cur)
    body = "\n".join("\n".join(x) for b in blocks for _, x in b)
    assert "scratch_" not in body or "Lb0EEEv" in lines[st], lines[st]  # spill-free product forms
    # one term: no group of these kernels reads a row's t1 half (byte 256 on)
    for b in blocks:
        for kd, sg in b:
            if kd == "asm" and any(x.startswith("v_mfma") for x in sg):
                assert not any(x.startswith("ds_read") and "offset:" in x and
                               int(x.rsplit("offset:", 1)[1]) >= 256 for x in sg), lines[st][:80]

    def succ(k):
        codes = [x for kd, sg in blocks[k] if kd == "gap" for x in sg]
        last = codes[-1] if codes else ""
        op = last.split()[0] if last else ""
        if op == "s_endpgm":
            return []
        if op == "s_branch":
            return [names[last.split()[1]]]
        out = [k + 1] if k + 1 < len(blocks) else []
        if op.startswith("s_cbranch"):
            out.append(names[last.split()[1]])
        return out

    def run(k, inflight, check):
        for kd, sg in blocks[k]:
            if kd == "asm":
                loads = [x for x in sg if x.startswith(("ds_read", "buffer_load"))]
                if any(x.startswith("v_mfma") for x in sg):
                    inflight = set()
                    for x in loads:
                        inflight |= _regs(x.split(",")[0])
                elif any(x.startswith("s_waitcnt vmcnt(0) lgkmcnt(0)") for x in sg):
                    inflight = None  # the drain
                elif loads:  # the prologue: its loads are in flight into the first group
                    inflight = set()
                    for x in loads:
                        inflight |= _regs(x.split(",")[0])
                continue
            if inflight is None:
                continue
            for x in sg:
                if check:
                    assert not (x.startswith("s_waitcnt") and "vmcnt" in x), (lines[st][:80], x)
                    assert not x.startswith("scratch_"), (lines[st][:80], x)
                    assert not (_regs(x) & inflight), (lines[st][:80], x)
        return inflight

    entry = [None] * len(blocks)
    reached = [False] * len(blocks)
    reached[0] = True
    work = [0]
    while work:  # forward dataflow to a fixpoint (states only grow)
        k = work.pop()
        out = run(k, entry[k], False)
        for n in succ(k):
            new = entry[n] if out is None else (set(out) | (entry[n] or set()))
            if not reached[n] or new != entry[n]:
                reached[n] = True
                entry[n] = new
                work.append(n)
    for k in range(len(blocks)):
        if reached[k]:
            run(k, entry[k], True)
    return sum(1 for b in blocks for kd, sg in b if kd == "asm" and any(x.startswith("v_mfma") for x in sg))
