"""Hostile memory around a launch: one arena, guard bands, poisoned outputs and workspaces, and the table of dense cases.

An Arena is ONE uint8 allocation.  Every tensor of a case is carved from it at a 256-byte-aligned address, with a guard band in
front of it and behind it (at least 256 rows of the widest row of the case, never less than 64 KiB), so that a tile read or written
past a tensor still lands inside the allocation: what such a kernel produces is a wrong value or a damaged guard, which a test
asserts on, and not a fault.  Everything is compared on integer views, so that NaN patterns compare equal to themselves.

tests/test_hostile_host.py runs the helper on CPU tensors and pins every case of the table on the route it is listed under (through
the planning hooks, without a device); tests/test_gpu_hostile_memory.py runs the cases."""
import ctypes

import numpy as np

ALIGN = 256
MIN_GUARD = 64 * 1024
GUARD_ROWS = 256
POISON = 0xFF     # NaN in fp16, bf16, fp32 and e4m3; -1 in int32
FRIENDLY = 0x00


def _up(n, a=ALIGN):
    return (int(n) + a - 1) // a * a


def as_bytes(torch, x):
    """flat uint8 tensor with the bytes of a numpy array or a torch tensor (on the tensor's device)"""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.contiguous().reshape(-1).view(torch.uint8)


def same_bits(torch, a, b):
    """bit identity of two tensors of equal dtype and shape (integer views: a NaN equals the same NaN)"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(as_bytes(torch, a), as_bytes(torch, b))


class Arena:
    """regions: [(name, nbytes, kind)] in address order, kind "in" (uploaded by the test, never to be written by a launch), "out"
    or "ws" (both filled by fill()).  row_bytes: the widest row of the case (head_dim x element size)."""

    def __init__(self, torch, regions, row_bytes, device="cuda"):
        self.torch = torch
        self.guard = _up(max(GUARD_ROWS * int(row_bytes), MIN_GUARD))
        self.regions = {}
        at = self.guard
        for name, nbytes, kind in regions:
            assert kind in ("in", "out", "ws") and name not in self.regions, (name, kind)
            self.regions[name] = (at, int(nbytes), kind)
            at = _up(at + int(nbytes)) + self.guard
        self.nbytes = at
        raw = torch.empty((self.nbytes + ALIGN,), dtype=torch.uint8, device=device)
        skew = (-raw.data_ptr()) % ALIGN
        self.buf = raw[skew:skew + self.nbytes]
        assert self.buf.data_ptr() % ALIGN == 0
        # the guard bands: everything that is no region (the padding behind a region's last byte included)
        self.spans = []
        at = 0
        for name, (off, nbytes, _) in self.regions.items():
            self.spans.append((at, off, "in front of " + name))
            at = off + nbytes
        self.spans.append((at, self.nbytes, "behind " + name))
        self.pattern = None

    def ptr(self, name):
        return self.buf.data_ptr() + self.regions[name][0]

    def size(self, name):
        return self.regions[name][1]

    def bytes(self, name):
        off, nbytes, _ = self.regions[name]
        return self.buf[off:off + nbytes]

    def view(self, name, dtype, shape):
        return self.bytes(name).view(dtype).reshape(shape)

    def upload(self, name, x):
        """copy x's bytes into the region; returns them (a tensor of their own on the arena's device) for unchanged()"""
        src = as_bytes(self.torch, x).to(self.buf.device)
        assert src.numel() == self.size(name), (name, src.numel(), self.size(name))
        self.bytes(name).copy_(src)
        return src.clone()

    def fill(self, pattern):
        """guards, outputs and workspace := pattern (one byte value); inputs stay"""
        for a, b, _ in self.spans:
            self.buf[a:b].fill_(pattern)
        for name, (_, _, kind) in self.regions.items():
            if kind != "in":
                self.bytes(name).fill_(pattern)
        self.pattern = pattern

    def damage(self):
        """[(which guard, byte offset into it, value found)]: the first damaged byte of every guard band that is not intact"""
        bad = []
        for a, b, what in self.spans:
            ne = self.buf[a:b] != self.pattern
            if bool(ne.any()):
                i = int(ne.to(self.torch.uint8).argmax())
                bad.append((what, i, int(self.buf[a + i])))
        return bad

    def guards_intact(self):
        return not self.damage()

    def unchanged(self, name, original_bytes):
        return self.torch.equal(self.bytes(name), original_bytes.to(self.buf.device))


# ------------------------------------------------------------------------------------------------------------------------------------
# The dense cases.  causal: 0 none, 1 top-left, 2 bottom-right (include/aule.h); window -1: none.
# how: "" the plain entry point | "rope" aule_attention_forward_rope_ex, tables in the arena | "min" the backward's minimum workspace
# (without the dS room).  Routes are what the planning hooks answer for the shape on a 256-CU device (tests/test_hostile_host.py).
DTYPE_CODE = {"fp32": 0, "fp16": 1, "bf16": 2}
ELEM = {"fp32": 4, "fp16": 2, "bf16": 2}

# (route, dtype, B, Hq, Hkv, Sq, Sk, D, causal, window, how)
FWD_CASES = [
    (0, "fp32", 1, 3, 3, 77, 201, 64, 1, -1, ""),            # no workspace
    (0, "fp32", 2, 4, 2, 129, 333, 32, 2, -1, ""),           # key-range pieces: 743 040 B of partials
    (1, "bf16", 1, 4, 2, 197, 203, 32, 1, -1, ""),
    (1, "fp16", 1, 6, 3, 97, 161, 64, 0, -1, ""),
    (1, "bf16", 1, 2, 2, 1, 1, 64, 0, -1, ""),               # B1 H2 S1 Sk1: nothing ragged
    (5, "fp16", 1, 8, 2, 13, 1999, 64, 0, -1, ""),
    (5, "bf16", 1, 8, 2, 13, 1999, 128, 2, -1, ""),
    (7, "bf16", 2, 4, 2, 333, 1100, 128, 2, -1, ""),         # 2.8 MB of partials
    (8, "fp16", 1, 4, 2, 515, 771, 64, 0, -1, ""),
    (8, "bf16", 1, 4, 4, 333, 333, 128, 1, -1, ""),
    (8, "bf16", 1, 4, 2, 515, 771, 128, 1, 200, ""),
    (8, "bf16", 1, 4, 2, 333, 1100, 128, 2, 300, ""),
    (8, "fp16", 1, 4, 2, 515, 771, 64, 0, -1, "rope"),
    (9, "fp16", 1, 4, 2, 257, 333, 256, 2, -1, ""),
    (9, "bf16", 1, 4, 1, 65, 1025, 256, 1, 100, ""),
    (9, "bf16", 2, 6, 2, 130, 129, 256, 0, 64, ""),          # a window without a causal mask: two query blocks, a ragged third key tile
    # route 4 is taken from the tiled split only with 32 units, at most 16 packed rows and 100 MB of K + V (short_query_route,
    # fa_fwd_gfx950.hip): 2 * 32 * Sk * 128 * 2 B >= 100e6 from Sk = 6104 on; 6105 is the first odd length
    (4, "bf16", 32, 1, 1, 1, 6105, 128, 0, -1, ""),
]

BWD_CASES = [
    (32, "fp32", 1, 3, 3, 77, 201, 64, 1, -1, ""),
    (32, "fp32", 2, 8, 2, 333, 700, 64, 1, -1, ""),          # small-grid pieces
    (128 | 32, "fp32", 1, 2, 1, 70, 150, 256, 1, -1, ""),
    (128, "bf16", 1, 4, 2, 70, 150, 256, 2, -1, ""),
    (128, "fp16", 1, 6, 2, 200, 300, 256, 1, 100, ""),       # two query blocks, three key blocks, a group of three, a window
    (8 | 16, "bf16", 1, 4, 4, 197, 203, 32, 1, -1, ""),
    (8 | 16, "bf16", 1, 4, 2, 130, 70, 128, 1, -1, ""),
    (8 | 16, "bf16", 1, 8, 2, 333, 1100, 128, 2, 300, ""),
    (1 | 4, "fp16", 1, 6, 3, 97, 161, 64, 0, -1, ""),
    (1 | 4, "bf16", 2, 8, 8, 515, 515, 128, 1, -1, ""),      # the dS room poisoned like the rest
    (2 | 16, "fp16", 2, 8, 2, 300, 300, 64, 0, -1, ""),
    (2 | 16, "fp16", 2, 8, 2, 515, 771, 64, 1, -1, ""),
    (4 | 8, "bf16", 1, 8, 8, 515, 515, 128, 1, 100, ""),
    (2 | 4, "fp16", 1, 6, 3, 97, 161, 64, 0, -1, "min"),
    # two key blocks per wave: more 128-key items than CUs and fewer rounds of 256-key items (bwd_dkv4_k2, fa_bwd_dkv4_gfx950.hip):
    # 32 units x 20 blocks = 640 items, 3 rounds of 256 CUs, against 320 items, 2 rounds
    (2 | 4 | 64, "bf16", 2, 32, 16, 515, 2500, 64, 0, -1, ""),
    (1 | 4, "bf16", 1, 2, 2, 1, 1, 64, 0, -1, ""),           # B1 H2 S1 Sk1: nothing ragged
    (1 | 4, "bf16", 1, 4, 2, 64, 1024, 128, 1, -1, ""),      # top-left, Sk >> Sq: keys 64 .. 1023 are seen by no query, dK = dV = 0 there
]


def case_id(c):
    route, dtype, B, Hq, Hkv, Sq, Sk, D, causal, window, how = c
    return "r%d-%s-B%dH%dkv%d-%dx%d-D%d-c%d-w%d%s" % (route, dtype, B, Hq, Hkv, Sq, Sk, D, causal, window, "-" + how if how else "")


def fill_problem(d, c, device=0):
    """the problem statement of an aule_attn_desc / aule_attn_bwd_desc (no pointers)"""
    _, dtype, B, Hq, Hkv, Sq, Sk, D, causal, window, _ = c
    d.struct_size = ctypes.sizeof(d)
    d.dtype = DTYPE_CODE[dtype]
    d.batch, d.heads_q, d.heads_kv, d.seq_q, d.seq_k, d.head_dim = B, Hq, Hkv, Sq, Sk, D
    d.scale, d.causal, d.window_size, d.device = D ** -0.5, causal, window, device
    return d


def ds_room_bytes(c):
    """the dS room of the 5-matmul backward: whole batch elements of DsLayout units at the workspace's end (as tests/test_gpu_bwd_plan.py)"""
    _, _, B, Hq, Hkv, Sq, Sk, _, _, _, _ = c
    return B * Hkv * 4 * ((Sk + 127) // 128) * (Hq // Hkv) * ((Sq + 31) // 32) * 2048


def bwd_workspace_bytes(lib, d, c):
    """workspace the case runs in: what the size query answers, or ("min") that without the dS room"""
    n = int(lib.aule_attention_backward_workspace_size(ctypes.byref(d)))
    return n - ds_room_bytes(c) if c[10] == "min" else n


def grad_close(got, ref, dtype, what):
    """tests/test_gpu_bwd.py::grad_close: |err| <= atol * max(1, max|grad|) + rtol * |ref| with util.BWD_TOL"""
    from util import BWD_TOL, assert_close
    atol, rtol = BWD_TOL[dtype]
    scale = max(1.0, float(np.abs(ref).max()))
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    print("%s: max|err| %.3e = %.2e of max|grad| %.3g  [bound %.1e * max(1, max|grad|) + %.0e * |ref|]"
          % (what, err.max(), err.max() / scale, scale, atol, rtol))
    assert_close(got, ref, atol * scale, rtol, what)
