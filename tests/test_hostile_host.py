"""tests/hostile.py without a device: the arena on CPU tensors (alignment, guard sizes, one flipped byte at every edge, integer
comparison of NaN patterns), and every dense case of its table planned on the route it is listed under (the planning hooks of
libaule.so need no device), so that a later change of the plan fails here instead of silently testing another kernel."""
import ctypes

import numpy as np
import pytest

import hostile
from hostile import ALIGN, BWD_CASES, FWD_CASES, MIN_GUARD, Arena, case_id


def _arena(torch, row_bytes=256):
    return Arena(torch, [("q", 1000, "in"), ("out", 77 * 6, "out"), ("none", 0, "ws"), ("ws", 4096, "ws")], row_bytes, device="cpu")


def test_regions_are_aligned_and_guarded():
    import torch
    for row_bytes in (64, 256, 1024):
        a = _arena(torch, row_bytes)
        assert a.guard >= MIN_GUARD and a.guard >= 256 * row_bytes and a.guard % ALIGN == 0
        end = 0
        for name in a.regions:
            off, nbytes, _ = a.regions[name]
            assert a.ptr(name) % ALIGN == 0 and a.ptr(name) == a.buf.data_ptr() + off
            assert off - end >= a.guard, "guard in front of " + name
            end = off + nbytes
        assert a.nbytes - end >= a.guard
        covered = sum(b - s for s, b, _ in a.spans) + sum(n for _, n, _ in a.regions.values())
        assert covered == a.nbytes, "guards and regions tile the allocation"
    assert _arena(torch, 1024).guard == 256 * 1024


def test_views_alias_the_arena():
    import torch
    a = _arena(torch)
    v = a.view("out", torch.bfloat16, (77, 3))
    v.fill_(1.5)
    assert v.data_ptr() == a.ptr("out") and bool((a.bytes("out").view(torch.bfloat16) == 1.5).all())
    assert a.view("none", torch.float32, (0,)).numel() == 0


@pytest.mark.parametrize("pattern", [0x00, 0xFF])
def test_one_flipped_byte_at_any_edge_is_seen(pattern):
    import torch
    a = _arena(torch)
    a.fill(pattern)
    assert a.guards_intact() and a.damage() == []
    edges = [0, a.nbytes - 1]
    for off, nbytes, _ in a.regions.values():
        edges += [off - 1, off + nbytes]
    for e in edges:
        a.buf[e] ^= 0x01
        assert not a.guards_intact(), e
        (what, i, found), = a.damage()
        assert found == pattern ^ 0x01
        a.buf[e] ^= 0x01
        assert a.guards_intact()
    # inside a region is no guard
    for name, (off, nbytes, _) in a.regions.items():
        if nbytes:
            a.buf[off] ^= 0x01
            a.buf[off + nbytes - 1] ^= 0x01
    assert a.guards_intact()


def test_fill_leaves_inputs_and_sets_the_rest():
    import torch
    a = _arena(torch)
    a.buf.fill_(0x11)
    orig = a.upload("q", np.arange(250, dtype=np.float32))
    a.fill(0xFF)
    assert a.unchanged("q", orig)
    assert bool((a.bytes("out") == 0xFF).all()) and bool((a.bytes("ws") == 0xFF).all())
    assert bool(torch.isnan(a.view("out", torch.float16, (-1,))).all()) and bool(torch.isnan(a.view("out", torch.bfloat16, (-1,))).all())
    assert bool(torch.isnan(a.view("ws", torch.float32, (-1,))).all()) and bool((a.view("ws", torch.int32, (-1,)) == -1).all())
    assert bool(torch.isnan(a.view("ws", torch.float8_e4m3fn, (-1,)).float()).all())
    a.bytes("q")[999] ^= 0x80
    assert not a.unchanged("q", orig)


def test_comparisons_are_made_on_integers():
    import torch
    a = _arena(torch)
    a.fill(0xFF)
    x = a.view("ws", torch.float32, (-1,))
    y = x.clone()
    assert not torch.equal(x, y), "NaN != NaN as floats"
    assert hostile.same_bits(torch, x, y) and a.unchanged("ws", hostile.as_bytes(torch, y))
    y.view(torch.int32)[5] = 0x7FC00000       # another NaN
    assert not hostile.same_bits(torch, x, y) and not a.unchanged("ws", hostile.as_bytes(torch, y))
    z = torch.zeros(4)
    assert not hostile.same_bits(torch, z, -z), "0.0 and -0.0 differ in bits"


def _lib():
    from aule import _capi
    return _capi, _capi.load()


@pytest.mark.parametrize("case", FWD_CASES, ids=case_id)
def test_forward_case_plans_its_route(case):
    _capi, lib = _lib()
    d = hostile.fill_problem(_capi.AttnDesc(), case)
    assert int(lib.aule_hip_debug_forward_route(ctypes.byref(d))) == case[0]
    if case[10] == "rope":
        r = _capi.AttnRope()
        r.struct_size = ctypes.sizeof(r)
        r.layout, r.table_len, r.table_pitch, r.q_pos_offset = _capi.ROPE_HALF, case[5], case[7] // 2, 0
        r.cos = r.sin = 4096       # (planned from the geometry; the pointers are looked at for null and alignment only)
        assert lib.aule_attention_forward_rope_fusable(ctypes.byref(d), ctypes.byref(r)) == 1


@pytest.mark.parametrize("case", BWD_CASES, ids=case_id)
def test_backward_case_plans_its_route(case):
    _capi, lib = _lib()
    d = hostile.fill_problem(_capi.AttnBwdDesc(), case)
    d.q = d.k = d.v = d.out = d.dout = d.lse = d.dq = d.dk = d.dv = d.workspace = 4096     # (never dereferenced by the plan)
    d.workspace_bytes = hostile.bwd_workspace_bytes(lib, d, case)
    assert int(lib.aule_hip_debug_backward_route(ctypes.byref(d))) == case[0]
    if case[10] == "min":                      # it IS the minimum, and with the dS room the same shape takes the 5-matmul mode
        d.workspace_bytes -= 1
        assert int(lib.aule_hip_debug_backward_route(ctypes.byref(d))) == -3
        assert (case[0] ^ 3,) + case[1:10] + ("",) in BWD_CASES


def test_the_tables_cover_every_route():
    assert {c[0] for c in FWD_CASES} == {0, 1, 4, 5, 7, 8, 9}
    bits = 0
    for c in BWD_CASES:
        bits |= c[0]
    assert bits == 255
    assert len({case_id(c) for c in FWD_CASES + BWD_CASES}) == len(FWD_CASES) + len(BWD_CASES)
