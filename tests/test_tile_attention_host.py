"""What the tiled ragged kernels share (csrc/fa_tile_attention.h, fa_varlen_common.h, fa_mla_prefill_common.h; DESIGN.md 3.8, 3.10,
3.11): source-text checks, no compiler and no GPU.  The dQ body, the score product, the 16-bit row store, the MLA tile source and
the host-side dispatch are written once and the kernels call them; the forward kernels keep their own softmax step (as shared
pieces they missed the resource and speed bars: profiles/tile_refactor_resources.txt, profiles/tile_refactor_ab.txt)."""
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "aule-attention_amd", "csrc")
FORWARD = ["fa_fwd_paged_prefill_gfx950.hip", "fa_fwd_paged_shared_prefix_gfx950.hip", "fa_fwd_varlen_gfx950.hip", "fa_fwd_mla_prefill_gfx950.hip"]
BACKWARD = ["fa_bwd_varlen_gfx950.hip", "fa_bwd_mla_prefill_gfx950.hip"]
HEADERS = ["fa_tile_attention.h", "fa_varlen_common.h", "fa_mla_prefill_common.h", "fa_paged_tile.h"]
# outside this family on purpose: the fp32 path of the D = 256 kernels and the cross-wave paged-MLA body
OWN_STEP = {"fa_fwd_d256_gfx950.hip", "fa_mla_common.h"}


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def _kernel_body(text, name):
    """the braces of the __global__ function `name`"""
    at = text.index("%s(const " % name)
    assert "__global__" in text[text.rindex("\n", 0, text.rindex("\n", 0, at)):at], name
    i = text.index("{", at)
    depth, j = 1, i + 1
    while depth:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        j += 1
    return text[i:j]


def test_the_shared_pieces_are_defined_once():
    tile, ragged, mla = _read("fa_tile_attention.h"), _read("fa_varlen_common.h"), _read("fa_mla_prefill_common.h")
    everything = "".join(_read(f) for f in FORWARD + BACKWARD + HEADERS)
    for name, count in (("tile_scores", 1), ("store_row16", 1), ("ragged_dq_body", 1)):
        assert len(re.findall(r"^__device__ __forceinline__ void %s\(" % name, everything, re.M)) == count, name
    assert len(re.findall(r"^int dispatch_tile_instance\(", everything, re.M)) == 2    # with and without the cache kind
    assert "void tile_scores(" in tile and "void store_row16(" in tile and "void ragged_dq_body(" in ragged
    for name in ("struct MlaKeyTiles", "constexpr int kDQK", "constexpr int kDN", "constexpr int kDR", "constexpr int kDV", "void mla_inputs("):
        assert everything.count(name) == 1 and name in mla, name
    for name in ("inline bool varlen_args_ok(", "inline int seqlen_cut("):
        assert _read("fa_kernels.h").count(name) == 1, name


def test_the_dq_kernels_are_one_body():
    for f, stem, shape in [(BACKWARD[0], "fa_bwd_varlen", "VarlenShape<D>"), (BACKWARD[1], "fa_bwd_mla", "MlaShape")]:
        text = _read(f)
        assert "ragged_dq_body<T, %s>(" % shape in _kernel_body(text, stem + "_dq_kernel"), f
        assert "store_row16<" in _kernel_body(text, stem + "_dkdv_kernel"), f
        # the dQ inner loop lives in the body alone
        assert "dp[kk][rr] - dl" not in text, f
    body = _read("fa_varlen_common.h")
    body = body[body.index("void ragged_dq_body("):]
    assert body.count("dp[kk][rr] - dl") == 1 and body.count("tile_scores<") == 2 and "store_row16<" in body and "query_block(" in body


def test_the_16_bit_row_store_of_the_backward_is_written_once():
    for f in (BACKWARD[0], "fa_varlen_common.h", "fa_mla_prefill_common.h"):
        assert "T::pack2(" not in _read(f), f
    assert _read("fa_tile_attention.h").count("T::pack2(") == 2     # one row store
    # what remains in the MLA backward: the dk_pe store, which is a 16-bit row or an fp32 plane by the plan's chunk count, and the reduce
    mla = _read(BACKWARD[1])
    assert mla.count("T::pack2(") == 6 and mla.count("T::pack2(a0, a1)") == 1 and "p.nchunks == 1" in mla
    assert mla.count("store_row16<") == 2 and _read(BACKWARD[0]).count("store_row16<") == 2


def test_one_dispatch_replaces_the_ladders():
    for f in FORWARD[:3] + BACKWARD[:1]:
        text = _read(f)
        assert text.count("dispatch_tile_instance(") == 1, f
        assert "launch_dim" not in text and "launch_kind" not in text and "launch_instance" not in text, f
    for f in (FORWARD[2], BACKWARD[0]):
        assert "varlen_args_ok(a)" in _read(f) and "token_stride %" not in _read(f), f


def test_where_the_softmax_step_is_written():
    """the four forward kernels keep their step; nothing else in csrc gains one"""
    have = {f for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc")) and "fast_exp2(m - mu)" in _read(f)}
    assert have == OWN_STEP | set(FORWARD), sorted(have)
    for f in FORWARD:
        assert _read(f).count("fast_exp2(m - mu)") == 1, f
