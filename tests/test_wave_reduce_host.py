"""Host checks of the written-out wave reductions (bpl-next_amd/csrc/wave_reduce.hip.h), no GPU needed:
the committed header is what tools/gen/wave_reduce_asm.py prints, every asm block computes what its comment
promises when run lane by lane (tests/dpp_emu.py) on the inputs the GPU probes use (tests/wave_cases.py), no DPP
read comes too soon after the write of its source, and every register written is declared."""
import contextlib
import io
import os
import runpy

import numpy as np
import pytest

import dpp_emu
import wave_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "bpl-next_amd", "csrc", "wave_reduce.hip.h")
GENERATOR = os.path.join(ROOT, "tools", "gen", "wave_reduce_asm.py")


@pytest.fixture(scope="module")
def blocks():
    return dpp_emu.parse(open(HEADER).read())


def test_committed_header_is_what_the_generator_prints():
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        runpy.run_path(GENERATOR, run_name="__main__")
    assert out.getvalue() == open(HEADER).read()


def test_every_function_is_parsed_with_the_signature_of_its_contract(blocks):
    assert set(blocks) == set(wc.CONTRACTS)
    for name, (nf, ops, where) in wc.CONTRACTS.items():
        b = blocks[name]
        assert (len(b.f32), len(b.f64)) == (nf, len(ops)), name
        assert {"lane63": "lane 63", "lane4": "lane 4", "row": "every lane of a row"}[where] in b.doc, name


def _lanes_of(where):
    return 8 if where == "lane4" else 64


def _promised(x, where):
    """The lanes the comment promises, as [n, k]: lane 63, lane 4, or all 64 (row totals)."""
    return x[:, 63:64] if where == "lane63" else x[:, 4:5] if where == "lane4" else x


def _row_or_wave(total_of, x, where):
    """Reference per promised lane: the wave's total, or every lane's own 16-lane row total."""
    if where == "row":
        return np.repeat(total_of(x.reshape(-1, 4, 16)), 16, axis=-1)
    return total_of(x)[:, None]


@pytest.mark.parametrize("name", sorted(wc.CONTRACTS))
def test_emulated_block_gives_the_exact_totals_and_maxima(blocks, name):
    nf, ops, where = wc.CONTRACTS[name]
    lanes = _lanes_of(where)
    # (all chains in ONE call, each with its own scale and placement; shorter case lists repeat)
    f_in = [wc.max_waves(c, f32=True, lanes=lanes) for c in range(nf)]
    d_in = [wc.max_waves(nf + c, lanes=lanes) if op == "max" else wc.sum_waves(c, lanes=lanes) for c, op in enumerate(ops)]
    n = max(len(x) for x in f_in + d_in)
    f_in = [np.resize(x, (n, 64)) for x in f_in]
    d_in = [np.resize(x, (n, 64)) for x in d_in]
    f_out, d_out = dpp_emu.run(blocks[name], f_in, d_in)
    for c in range(nf):
        wc.assert_bits_equal(_promised(f_out[c], where), f_in[c].max(axis=-1)[:, None], f"{name} float chain {c}")
    for c, op in enumerate(ops):
        if op == "max":
            want = _row_or_wave(lambda x: x.max(axis=-1), d_in[c], where)
        else:
            want = _row_or_wave(wc.int_sum, d_in[c], where).astype(np.float64)
        wc.assert_bits_equal(_promised(d_out[c], where), want, f"{name} double chain {c} ({op})")


@pytest.mark.parametrize("name", sorted(n for n, c in wc.CONTRACTS.items() if "add" in c[1]))
def test_emulated_sums_of_normals_stay_within_the_pairwise_bound(blocks, name):
    nf, ops, where = wc.CONTRACTS[name]
    lanes = _lanes_of(where)
    f_in = [np.resize(wc.max_waves(c, f32=True, lanes=lanes), (16, 64)) for c in range(nf)]
    d_in = [np.resize(wc.max_waves(nf + c, lanes=lanes), (16, 64)) if op == "max" else wc.normal_waves(c, lanes=lanes)
            for c, op in enumerate(ops)]
    _, d_out = dpp_emu.run(blocks[name], f_in, d_in)
    for c, op in enumerate(ops):
        if op == "add":
            x = d_in[c].reshape(-1, 4, 16) if where == "row" else d_in[c]
            want, mag = wc.fsum_last(x)
            if where == "row":
                want, mag = np.repeat(want, 16, axis=-1), np.repeat(mag, 16, axis=-1)
            else:
                want, mag = want[:, None], mag[:, None]
            assert (np.abs(_promised(d_out[c], where) - want) <= 6 * 2.0 ** -53 * mag).all(), (name, c)


@pytest.mark.parametrize("name", sorted(wc.CONTRACTS))
def test_no_dpp_read_within_two_wait_states_of_the_write(blocks, name):
    assert dpp_emu.hazards(blocks[name]) == []


@pytest.mark.parametrize("name", sorted(wc.CONTRACTS))
def test_every_register_written_is_an_operand_or_a_clobber(blocks, name):
    assert dpp_emu.undeclared_writes(blocks[name]) == []


def test_emulator_refuses_what_it_does_not_implement():
    for text in ("v_add_f32 v1, v2, v3", "v_mov_b32_dpp v1, v2 row_shr:1 row_mask:0xf bank_mask:0xf",
                 "v_mov_b32_dpp v1, v2 row_ror:4 row_mask:0xf bank_mask:0x3", "v_add_f64 v[31:32], v[30:31], v[32:33]"):
        with pytest.raises(ValueError):
            dpp_emu._ins(text)


def test_hazard_and_clobber_checks_see_a_planted_defect(blocks):
    """The static checks on doctored copies of a real block: a dropped s_nop and a dropped clobber are reported."""
    b = blocks["wave_reduce_sum1_f64_raw"]
    prog = list(b.program)
    del prog[4]                                   # the s_nop 1 between the first add and the next DPP read
    assert b.program[4].op == "s_nop" and dpp_emu.hazards(b._replace(program=tuple(prog))) != []
    assert dpp_emu.undeclared_writes(b._replace(clobbers=b.clobbers[1:])) == [b.clobbers[0]]
