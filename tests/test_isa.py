"""CPU check of the built library's gfx950 code (no GPU): the pipelined
gathering kernel's counted wait (linearize_gather_kernel, gn/gather.h) is only
correct if at least NPL vector-memory operations follow the 8 LDS-DMA refill
loads on every path back to the loop top's `s_waitcnt vmcnt(NPL)` (vmcnt counts
in issue order; the inline-asm LDS reads of the slot are invisible to the
compiler's own waits). The compiler could sink, split or merge the plane
stores that follow the refill; this test disassembles the code object in
libm3s_gn.so and checks every branch to, and every fall-through into, such a
wait."""
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "mast3r-slam-ysh_amd", "mast3r_slam_backends", "libm3s_gn.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
NPL = {0: 4, 1: 4, 2: 3}  # planes per mode: points, rays, calib (PixIn<MODE>::kPlanes)


def code_object(path):
    data = open(path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    i = data.find(magic)
    assert i >= 0, "no offload bundle in the library"
    n = struct.unpack_from("<Q", data, i + 24)[0]
    off = i + 32
    for _ in range(n):
        o, sz, tl = struct.unpack_from("<QQQ", data, off)
        trip = data[off + 24:off + 24 + tl].decode()
        off += 24 + tl
        if "gfx950" in trip:
            return data[i + o:i + o + sz]
    raise AssertionError("no gfx950 code object")


@pytest.fixture(scope="module")
def disasm(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(OBJDUMP)):
        pytest.skip("library or llvm-objdump missing")
    co = tmp_path_factory.mktemp("isa") / "gn.co"
    co.write_bytes(code_object(LIB))
    return subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", str(co)], check=True, capture_output=True,
                          text=True).stdout


def kernel_insns(text, mode):
    """[(address, instruction)] of linearize_gather_kernel<mode>."""
    name = f"linearize_gather_kernelILi{mode}EEEvNS_7LinArgsE>:"
    lines = text.splitlines()
    start = next(i for i, l in enumerate(lines) if l.endswith(name))
    out = []
    for l in lines[start + 1:]:
        if re.match(r"^[0-9a-f]+ <", l):
            break
        m = re.search(r"//\s*([0-9A-Fa-f]+):?", l)
        if m and l.strip():
            out.append((int(m.group(1), 16), l.split("//")[0].strip()))
    return out


VMEM = re.compile(r"^(global|buffer|flat)_(load|store|atomic)")


@pytest.mark.parametrize("mode", [1, 2])
def test_gather_refill_is_covered_by_counted_wait(disasm, mode):
    ins = kernel_insns(disasm, mode)
    npl = NPL[mode]
    addr_idx = {a: i for i, (a, _) in enumerate(ins)}
    waits = [i for i, (_, t) in enumerate(ins) if t == f"s_waitcnt vmcnt({npl})"]
    assert waits, "the loop top's counted wait is missing"
    lds = [i for i, (_, t) in enumerate(ins) if VMEM.match(t) and t.endswith(" lds")]
    assert lds, "no LDS-DMA refill found"

    def vmem_after_last_refill(end):  # scanning back from instruction `end` (exclusive)
        n = 0
        for j in range(end - 1, -1, -1):
            t = ins[j][1]
            if VMEM.match(t):
                if t.endswith(" lds"):
                    return n
                n += 1
            if t.startswith("s_endpgm"):
                return None
        return None

    checked = 0
    for w in waits:
        wa = ins[w][0]
        # branches landing at the wait (or on the instructions right before it
        # in the same block: s_waitcnt lgkmcnt / s_nop / moves)
        for j, (a, t) in enumerate(ins):
            m = re.match(r"^s_(c?branch\w*)\s", t)
            if not m:
                continue
            tgt = re.search(r"<[^+]+\+0x([0-9a-f]+)>", disasm_line(disasm, a))
            if not tgt:
                continue
            base = ins[0][0] - 0x0  # the function's first instruction address
            ta = kernel_base(disasm, mode) + int(tgt.group(1), 16)
            if ta in addr_idx and addr_idx[ta] <= w and all(not VMEM.match(ins[q][1]) and not ins[q][1].startswith("s_c")
                                                          for q in range(addr_idx[ta], w)):
                n = vmem_after_last_refill(j)
                if n is not None:
                    assert n >= npl, (mode, hex(a), n)
                    checked += 1
        # fall-through into the wait
        if w > 0 and not ins[w - 1][1].startswith("s_branch"):
            n = vmem_after_last_refill(w)
            if n is not None:
                assert n >= npl, (mode, hex(wa), n)
                checked += 1
    print(f"mode {mode}: {checked} paths into the counted wait checked")
    assert checked >= 1


_LINES = {}


def disasm_line(text, addr):
    if not _LINES:
        for l in text.splitlines():
            m = re.search(r"//\s*([0-9A-Fa-f]+):?", l)
            if m:
                _LINES[int(m.group(1), 16)] = l
    return _LINES.get(addr, "")


def kernel_base(text, mode):
    name = f"linearize_gather_kernelILi{mode}EEEvNS_7LinArgsE>:"
    for l in text.splitlines():
        if l.endswith(name):
            return int(l.split()[0], 16)
    raise AssertionError(name)


# ------------------------------------------------------------ poll loops --
# Every cross-workgroup wait in the library is a loop that re-reads a flag or
# a tagged granule until it changes. If the compiler hoists the read out of
# the loop (a plain read-only load in a loop that stores nothing may be), the
# wait can only time out: round 4 saw exactly that in the tracker once its
# s_sleep was removed (profiles/r04/trk_ab_sleep0_INVALID.txt). The loads are
# now poll_b128 (gn/llt_blocks.h: a compiler memory barrier in front of each) or
# agent-scope atomics. These tests find the loops in the machine code (natural
# loops of the control-flow graph) and check that each one reads memory.

POLL_READ = re.compile(r"^(buffer|global|flat)_(load|atomic)|^ds_(read|load|add_rtn|cmpst)")
SC1_LOAD = re.compile(r"^buffer_load_dword\w*\s.*\bsc1\b")
POLL_KERNELS = ("df_factor_kernel", "col_backsub_kernel", "tail_cyc_kernel", "tail_pair_kernel",
                "sparse_llt_kernel", "track_persistent_kernel")
TRK_SPINS = "0x400000"  # kTrkSpins = 1 << 22: the tracker's bounded-wait compare


def functions(text):
    """{symbol: [(address, instruction, branch-target offset or None)]}."""
    out, cur = {}, None
    for l in text.splitlines():
        m = re.match(r"^([0-9a-f]+) <(.*)>:$", l)
        if m:
            cur = m.group(2)
            out[cur] = []
            continue
        if cur is None or not l.strip():
            continue
        m = re.search(r"//\s*([0-9A-Fa-f]+):?", l)
        if m:
            t = re.search(r"<[^+>]+\+0x([0-9a-f]+)>", l)
            out[cur].append((int(m.group(1), 16), l.split("//")[0].strip(), int(t.group(1), 16) if t else None))
    return out


def natural_loops(ins):
    """(blocks [(first, end)], loops [(header, {blocks})]) of one function."""
    base = ins[0][0]
    at = {a: i for i, (a, _, _) in enumerate(ins)}
    starts = {0}
    for i, (_, t, off) in enumerate(ins):
        if re.match(r"^s_(c?branch|endpgm|setpc)", t):
            if i + 1 < len(ins):
                starts.add(i + 1)
            if off is not None and base + off in at:
                starts.add(at[base + off])
    starts = sorted(starts)
    blocks = [(s, starts[k + 1] if k + 1 < len(starts) else len(ins)) for k, s in enumerate(starts)]
    bid = {s: k for k, (s, _) in enumerate(blocks)}
    succ = [set() for _ in blocks]
    for k, (s, e) in enumerate(blocks):
        _, t, off = ins[e - 1]
        if off is not None and re.match(r"^s_c?branch", t) and base + off in at:
            succ[k].add(bid[at[base + off]])
        if not re.match(r"^s_(branch|endpgm|setpc)", t) and e < len(ins):
            succ[k].add(k + 1)
    pred = [set() for _ in blocks]
    for u, vs in enumerate(succ):
        for v in vs:
            pred[v].add(u)
    reach, st = set(), [0]
    while st:
        u = st.pop()
        if u not in reach:
            reach.add(u)
            st += list(succ[u])
    dom = {u: set(reach) for u in reach}
    dom[0] = {0}
    changed = True
    while changed:
        changed = False
        for u in sorted(reach - {0}):
            ps = [dom[p] for p in pred[u] if p in reach]
            nd = (set.intersection(*ps) if ps else set()) | {u}
            if nd != dom[u]:
                dom[u], changed = nd, True
    loops = []
    for u in reach:
        for h in succ[u]:
            if h in dom[u]:  # back edge u -> h
                body, st = {h}, [u]
                while st:
                    x = st.pop()
                    if x not in body:
                        body.add(x)
                        st += [p for p in pred[x] if p in reach]
                loops.append((h, body))
    return blocks, loops


def loops_marked(ins, marker):
    """For every block holding an instruction that satisfies `marker`: the
    instructions of the innermost natural loop around it."""
    blocks, loops = natural_loops(ins)
    out = []
    for k, (s, e) in enumerate(blocks):
        if any(marker(ins[i][1]) for i in range(s, e)):
            around = [b for _, b in loops if k in b]
            body = min(around, key=len) if around else {k}
            out.append((ins[s][0], [ins[i][1] for q in sorted(body) for i in range(*blocks[q])]))
    return out


def test_every_poll_loop_reads_memory(disasm):
    """Every loop of the solver and tracker kernels that waits (s_sleep) also
    reads: the flag / granule it waits on is loaded on every pass."""
    fns = functions(disasm)
    seen = {k: 0 for k in POLL_KERNELS}
    for name, ins in fns.items():
        kern = next((k for k in POLL_KERNELS if k in name), None)
        if kern is None or not ins:
            continue
        for addr, body in loops_marked(ins, lambda t: t.startswith("s_sleep")):
            assert any(POLL_READ.match(t) for t in body), f"{name}: wait loop at {addr:#x} reads nothing"
            seen[kern] += 1
        if kern == "track_persistent_kernel":  # its three granule polls: 16-B sc1 buffer loads
            polls = loops_marked(ins, lambda t: t.startswith("s_cmp") and TRK_SPINS in t)
            assert len(polls) >= 3, (name, len(polls))
            for addr, body in polls:
                assert any(SC1_LOAD.match(t) for t in body), f"{name}: poll at {addr:#x} has no sc1 load"
    assert all(seen.values()), seen


def test_tracker_polls_keep_their_loads_without_sleep(tmp_path):
    """The round-4 failure mode itself: the tracker built without the s_sleep
    in its polls (-DM3S_TRK_SLEEP=0). Each bounded-wait loop must still hold
    its granule load (with poll_b128's barrier removed, -DM3S_POLL_BARRIER=0,
    the compiler hoists the partial and shard-sum loads out of the loop:
    checked when this test was written, round 5)."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not (os.path.exists(hipcc) and os.path.exists(OBJDUMP)):
        pytest.skip("hipcc or llvm-objdump missing")
    src = os.path.join(ROOT, "mast3r-slam-ysh_amd", "csrc", "m3s_gn.hip")
    obj = tmp_path / "nosleep.o"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", "--cuda-device-only",
                    "--no-gpu-bundle-output", "-c", "-DM3S_TRK_SLEEP=0", "-I", os.path.join(ROOT, "include"), src,
                    "-o", str(obj)], check=True, capture_output=True)
    text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", str(obj)], check=True, capture_output=True,
                          text=True).stdout
    n = 0
    for name, ins in functions(text).items():
        if "track_persistent_kernel" not in name or not ins:
            continue
        polls = loops_marked(ins, lambda t: t.startswith("s_cmp") and TRK_SPINS in t)
        assert len(polls) >= 3, (name, len(polls))
        for addr, body in polls:
            assert any(SC1_LOAD.match(t) for t in body), f"{name}: poll at {addr:#x} lost its load"
        n += 1
    assert n >= 8, n


# ------------------------------------------------- packed-kernel VALU budget --
# Round 5 (tools/isa_loop.py): the calib trip of
# linearize_packed_kernel<2> executes 268 VALU instructions per 4-pixel trip
# (283 in round 4, where a partial-trip guard had been merged into per-lane
# selects on every trip). This pins the count so that such a regression shows
# up here instead of in a round's timing: the innermost natural loop around the
# trip's LDS-DMA refill, without the blocks of the partial trip's own refill
# (sc0 loads, taken at most once per wave).
@pytest.mark.parametrize("mode,budget", [(2, 268), (1, 324), (0, 171)])
def test_packed_trip_valu_budget(disasm, mode, budget):
    fns = functions(disasm)
    name = next(n for n in fns if f"linearize_packed_kernelILi{mode}EEEvNS_7LinArgsE" in n)
    ins = fns[name]
    blocks, loops = natural_loops(ins)
    refill = [k for k, (s, e) in enumerate(blocks)
              if any(VMEM.match(ins[i][1]) and ins[i][1].endswith(" nt lds") for i in range(s, e))]
    assert refill, "no LDS-DMA refill in the packed kernel"
    def has_pk(b):
        return any(ins[i][1].startswith("v_pk_fma_f32") for q in b for i in range(*blocks[q]))
    around = [b for _, b in loops if any(k in b for k in refill) and has_pk(b)]
    assert around, "no trip loop around the refill"
    body = min(around, key=len)
    rare = {q for q in body if any(ins[i][1].endswith(" sc0 lds") for i in range(*blocks[q]))}
    valu = sum(1 for q in body - rare for i in range(*blocks[q]) if ins[i][1].startswith("v_"))
    print(f"mode {mode}: {valu} VALU per trip in the loop's common blocks")
    assert valu <= budget, (mode, valu, budget)
