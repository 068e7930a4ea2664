"""The one-term K loop (AZ_CONV_F16; gen_kloop_asm.group_asm_h /
prologue_asm_h -> KGroupH / KProH / KDrainH) on test_kloop_schedule_cpu's
symbolic machine: every form the one-term kernels instantiate, under every
skip word, sequenced as az_tower16.hip's k_loop_asm sequences it (prologue,
the projection's group, 9 tap groups, drain).

Each accumulator must see every unskipped k-step's single product t0 * B0
exactly once and in k-step order -- N block 0 from fragment 0, N block 1
from fragment 2 -- from landed registers of the right k-step, tap, block and
chunk; no load of fragment 1 or 3 and no read of a row's t1 half is ever
issued; nothing is in flight after the drain; and the emitter's WAR rule
holds: between the last MFMA that reads a register and a load that targets
it lie at least WAR_GAP other MFMAs or an s_nop of at least 4."""
import re
from collections import Counter

import pytest

from test_kloop_schedule_cpu import FORMS, SKIPS, Machine, gen

# (blocks per wave, first chunk, prefetch depth, residual steps) of the one-term kernels: k_loop_asm's
# PF per form (2, the 6-block waves and the stem's 2-k-step groups 1) over gen.H_FORMS
H_FORMS = [(mbw, c0, pf, r) for mbw, forms in gen.H_FORMS.items() for c0, pf in forms for r in ((0, 4) if c0 == 0 else (0,))]


def test_forms_are_the_three_term_kernels_forms():
    # each is a form of the three-term table too: the same tiles, the same prefetch depths
    assert set(H_FORMS) <= set(FORMS) and len(H_FORMS) == 10


def sequence(MBW, C0, PF, R, skw):
    """[(text, ctx)] of one K loop, the last tap with HN = 1 as k_loop_asm runs it."""
    first_src = ("own",) if R else ("tap", 0)
    first_k = ("R", 0) if R else ("M", C0)
    seq = [(gen.prologue_asm_h(MBW, C0, PF), {"sc": first_k, "d": first_src, "skip": 0, "acc": "-", "rc": first_k[0]})]
    if R:
        seq.append((gen.group_asm_h(MBW, 0, 0, PF, 1), {"sc": ("R", 0), "sn": ("M", 0), "d": ("own",), "n": ("tap", 0),
                                                        "skip": 0, "acc": "res", "rc": "R", "rn": "M"}))
    for t in range(9):
        skc = (skw >> (2 * t)) & 3
        nxt = ("tap", t + 1) if t < 8 else ("tap", 8)
        sn = ("M", 4 * (t + 1) + C0) if t < 8 else ("M", 4 * t + C0)
        seq.append((gen.group_asm_h(MBW, C0, skc, PF, 1), {"sc": ("M", 4 * t), "sn": sn, "d": ("tap", t), "n": nxt,
                                                           "skip": skc, "acc": "main", "rc": "M", "rn": "M"}))
    return seq


def check_war(texts):
    """The WAR rule over the whole loop's instruction stream."""
    mf, reader = 0, {}
    for text in texts:
        for line in text.split("\\n\\t"):
            ops = re.findall(r"%\[(\w+)\]", line)
            if line.startswith("v_mfma"):
                mf += 1
                reader[ops[1]] = reader[ops[2]] = mf
            elif line.startswith("s_nop"):
                if int(line.split()[1]) >= 4:
                    reader.clear()
            elif line.startswith(("ds_read", "buffer_load")):
                assert ops[0] not in reader or mf - reader[ops[0]] >= gen.WAR_GAP, (line, mf - reader[ops[0]])


@pytest.mark.parametrize("MBW,C0,PF,R", H_FORMS)
@pytest.mark.parametrize("skw", SKIPS)
def test_one_term_schedule_is_exact(MBW, C0, PF, R, skw):
    m = Machine(MBW)
    seq = sequence(MBW, C0, PF, R, skw)
    for text, ctx in seq:
        # one term, the main fragments: nothing else is ever loaded or read
        for line in text.split("\\n\\t"):
            if line.startswith("buffer_load"):
                assert int(line.rsplit("offset:", 1)[1]) in (0, 2048), line
            if line.startswith("ds_read"):
                assert int(line.rsplit("offset:", 1)[1]) < 256, line
        m.run(text, ctx)
    check_war([t for t, _ in seq])
    # the drain (s_waitcnt vmcnt(0) lgkmcnt(0)): the last tap's prefetch of its own first k-steps lands
    m.land(m.vm, 0)
    m.land(m.lgkm, 0)
    assert not m.vm and not m.lgkm
    for blk in range(MBW):
        for n in range(2):
            want = Counter()
            for t in range(9):
                if ((skw >> (2 * t)) & 3) >> blk & 1:
                    continue
                for c in range(C0, 4):
                    want[(("M", 4 * t + c), 2 * n, 0, n)] += 1  # fragment 0 / 2, term 0
            assert m.acc.get(("main", blk, n), Counter()) == want, (blk, n)
            seq_k = [x[0] for x in m.seq.get(("main", blk, n), [])]
            assert seq_k == sorted(seq_k)
            if R:
                want = Counter({(("R", c), 2 * n, 0, n): 1 for c in range(4)})
                assert m.acc.get(("res", blk, n), Counter()) == want, (blk, n, "residual")
                seq_k = [x[0] for x in m.seq[("res", blk, n)]]
                assert seq_k == sorted(seq_k)


def test_war_check_sees_a_short_distance():
    """The rule's check is live: a read moved right behind its slot's pair fails it."""
    text = gen.group_asm_h(4, 0, 0, 2, 1)
    lines = text.split("\\n\\t")
    i = next(j for j, l in enumerate(lines) if l.startswith("ds_read_b128 %[a0_0]"))
    pair_end = max(j for j in range(i) if lines[j].startswith("v_mfma") and "%[a0_0]" in lines[j])
    lines.insert(pair_end + 1, lines.pop(i))
    with pytest.raises(AssertionError):
        check_war(["\\n\\t".join(lines)])
    check_war([text])
