"""A lane-level emulator of the written-out wave reductions (bpl-next_amd/csrc/wave_reduce.hip.h).

parse() reads the inline-asm blocks out of the header text; run() executes one block on [n, 64] lanes;
hazards() and undeclared_writes() are static checks over the same parsed program.  Exactly the mnemonics and
DPP controls the generator emits are implemented -- anything else raises, so a regenerated header that uses a
new form fails loudly here instead of being emulated wrongly.

DPP semantics (CDNA ISA, "Data Parallel Primitives"): lane i of a 16-lane row reads src0 from
    quad_perm:[a,b,c,d]  lane (i & ~3) + [a,b,c,d][i & 3]
    row_ror:n            lane i - n of its own row (rotating)
    row_bcast:15         lane 15 of the row below (row 0 has no source)
    row_bcast:31         lane 31 (rows 0 and 1 have no source)
and a lane without a source, or whose row is not in row_mask, keeps its old destination (bound_ctrl is off).
"""
import re
from collections import namedtuple

import numpy as np

Ins = namedtuple("Ins", "op dst srcs ctrl row_mask text")
Block = namedtuple("Block", "name doc f32 f64 operands clobbers program")

_FUNC = re.compile(r"((?://[^\n]*\n)+)__device__ __forceinline__ void (\w+)\(([^)]*)\) \{\s*asm volatile\((.*?)\);\s*\}", re.S)
_REG = r"v(\d+)|v\[(\d+):(\d+)\]"


def _regs(tok):
    m = re.fullmatch(_REG, tok.strip())
    if not m:
        raise ValueError(f"not a VGPR operand: {tok!r}")
    if m.group(1) is not None:
        return (int(m.group(1)),)
    lo, hi = int(m.group(2)), int(m.group(3))
    if hi != lo + 1 or lo & 1:
        raise ValueError(f"not an aligned register pair: {tok!r}")
    return (lo, hi)


def _ins(text):
    if re.fullmatch(r"s_nop \d+", text):
        return Ins("s_nop", (), (), int(text.split()[1]), 0xF, text)
    m = re.fullmatch(r"(v_mov_b32_dpp|v_max_f32_dpp) (.*?) ((?:quad_perm|row_ror|row_bcast)\S+) row_mask:0x([0-9a-f]) bank_mask:0xf", text)
    if m:
        ops = [_regs(t) for t in m.group(2).split(",")]
        if len(ops) != (2 if m.group(1) == "v_mov_b32_dpp" else 3) or any(len(o) != 1 for o in ops):
            raise ValueError(f"operands: {text!r}")
        c = m.group(3)
        q = re.fullmatch(r"quad_perm:\[([0-3]),([0-3]),([0-3]),([0-3])\]", c)
        if q:
            ctrl = ("quad_perm", tuple(int(g) for g in q.groups()))
        elif c in ("row_ror:4", "row_ror:8"):
            ctrl = ("row_ror", int(c[-1]))
        elif c in ("row_bcast:15", "row_bcast:31"):
            ctrl = ("row_bcast", int(c[-2:]))
        else:
            raise ValueError(f"DPP control not emulated: {text!r}")
        return Ins(m.group(1), ops[0], tuple(o[0] for o in ops[1:]), ctrl, int(m.group(4), 16), text)
    m = re.fullmatch(r"(v_add_f64|v_max_f64) (v\[\d+:\d+\]), (v\[\d+:\d+\]), (v\[\d+:\d+\])", text)
    if m:
        return Ins(m.group(1), _regs(m.group(2)), (_regs(m.group(3)), _regs(m.group(4))), None, 0xF, text)
    raise ValueError(f"instruction not emulated: {text!r}")


def parse(header_text):
    """{function name: Block} for every asm block of the header."""
    blocks = {}
    for doc, name, args, body in _FUNC.findall(header_text):
        code, tail = re.split(r"\n\s*:", body, maxsplit=1)
        lines = re.findall(r'^\s*"(.*)\\n\\t"$', code, re.M)
        if len(lines) != len([ln for ln in code.splitlines() if ln.strip()]):
            raise ValueError(f"{name}: a line of the asm block is not one quoted instruction")
        parts = re.split(r"\n\s*:", tail)
        outs = re.findall(r'"\+\{(v\d+|v\[\d+:\d+\])\}"\((\w+)\)', parts[0])
        if len(parts) not in (1, 3) or (len(parts) == 3 and parts[1].strip()):
            raise ValueError(f"{name}: operand lists")
        clob = tuple(int(r) for r in re.findall(r'"v(\d+)"', parts[2])) if len(parts) == 3 else ()
        params = [(t, n) for t, n in re.findall(r"(float|double)& (\w+)", args)]
        if [n for _, n in params] != [n for _, n in outs]:
            raise ValueError(f"{name}: operands do not follow the parameters")
        operands = tuple((_regs(r), t) for (r, _), (t, _) in zip(outs, params))
        for regs, t in operands:
            if len(regs) != (1 if t == "float" else 2):
                raise ValueError(f"{name}: operand width")
        blocks[name] = Block(name, doc, tuple(r[0] for r, t in operands if t == "float"),
                             tuple(r for r, t in operands if t == "double"), operands, clob,
                             tuple(_ins(ln) for ln in lines))
    return blocks


def _source_lanes(ctrl):
    """(source lane of every lane, has-a-source mask)."""
    i = np.arange(64)
    kind, arg = ctrl
    if kind == "quad_perm":
        return (i & ~3) + np.array(arg)[i & 3], np.ones(64, bool)
    if kind == "row_ror":
        return (i & ~15) + ((i & 15) - arg) % 16, np.ones(64, bool)
    if arg == 15:
        return np.maximum((i & ~15) - 1, 0), i >= 16
    return np.full(64, 31), i >= 32


def _f64(regs, pair):
    return ((regs[pair[1]].astype(np.uint64) << np.uint64(32)) | regs[pair[0]].astype(np.uint64)).view(np.float64)


def run(block, f32_in, f64_in):
    """Execute one block.  f32_in / f64_in: one [n, 64] array per float / double parameter, in the order of the
    signature.  Returns (f32_out, f64_out) in the same form: what every lane holds at the end."""
    if len(f32_in) != len(block.f32) or len(f64_in) != len(block.f64):
        raise ValueError(f"{block.name}: {len(block.f32)} floats and {len(block.f64)} doubles")
    regs = {}
    for r, x in zip(block.f32, f32_in):
        regs[r] = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    for (lo, hi), x in zip(block.f64, f64_in):
        bits = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
        regs[lo] = (bits & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        regs[hi] = (bits >> np.uint64(32)).astype(np.uint32)
    shape = next(iter(regs.values())).shape
    rs = np.random.RandomState(1)
    for r in block.clobbers:   # (a temporary holds anything on entry)
        regs[r] = rs.randint(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    with np.errstate(all="ignore"):
        for ins in block.program:
            if ins.op == "s_nop":
                continue
            for s in np.ravel(ins.srcs):
                if s not in regs:
                    raise ValueError(f"{block.name}: v{s} read before anything wrote it: {ins.text}")
            if ins.op in ("v_add_f64", "v_max_f64"):
                a, b = _f64(regs, ins.srcs[0]), _f64(regs, ins.srcs[1])
                bits = (a + b if ins.op == "v_add_f64" else np.maximum(a, b)).view(np.uint64)
                regs[ins.dst[0]] = (bits & np.uint64(0xFFFFFFFF)).astype(np.uint32)
                regs[ins.dst[1]] = (bits >> np.uint64(32)).astype(np.uint32)
                continue
            src, has = _source_lanes(ins.ctrl)
            live = has & (((ins.row_mask >> (np.arange(64) >> 4)) & 1) == 1)
            moved = regs[ins.srcs[0]][..., src]
            if ins.op == "v_max_f32_dpp":
                moved = np.maximum(moved.view(np.float32), regs[ins.srcs[1]].view(np.float32)).view(np.uint32)
            old = regs.get(ins.dst[0])
            if old is None:
                if not live.all():
                    raise ValueError(f"{block.name}: v{ins.dst[0]} partly written before it holds anything: {ins.text}")
                old = moved
            regs[ins.dst[0]] = np.where(live, moved, old)
    return [regs[r].view(np.float32) for r in block.f32], [_f64(regs, p) for p in block.f64]


def _writes(ins):
    return set(ins.dst)


def hazards(block):
    """Instructions that read a VGPR through a DPP control less than two wait states after a VALU instruction
    wrote it (s_nop N counts N + 1; the operands count as written right before the block)."""
    bad = []
    last_write = {r: -1 for regs, _ in block.operands for r in regs}   # wait-state clock of the last VALU write
    clock = 0
    for ins in block.program:
        if ins.op == "s_nop":
            clock += ins.ctrl + 1
            continue
        if ins.ctrl is not None:
            r = ins.srcs[0]
            if r in last_write and clock - last_write[r] - 1 < 2:
                bad.append(ins.text)
        for r in _writes(ins):
            last_write[r] = clock
        clock += 1
    return bad


def undeclared_writes(block):
    """Registers the block writes that are neither an in/out operand nor in the clobber list."""
    declared = {r for regs, _ in block.operands for r in regs} | set(block.clobbers)
    return sorted({r for ins in block.program for r in _writes(ins)} - declared)
