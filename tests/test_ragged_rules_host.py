"""The rules every ragged serving kernel shares are written once: source-text checks over the code lines of csrc/
(comments stripped), no compiler and no GPU; and the clamp property itself, on the host, under ASan + UBSan (a stand-alone program:
tests/ragged_clamps_main.cpp).  The device code these helpers compile to is compared with the hand-written statements' in
profiles/ragged_rules_resources.txt."""
import os
import re
import subprocess

from conftest import ROOT
from util import makefile_compile_line

CSRC = os.path.join(ROOT, "aule-attention_amd", "csrc")
# call sites that keep a hand-written statement because the shared one changed their instruction stream: none
HAND_WRITTEN = {}


def _code(name):
    """the file without its comments"""
    text = open(os.path.join(CSRC, name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _sources():
    return {f: _code(f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h", ".cpp")) or f == "fa_fwd_splitkv_body.inc"}


def _function(text, head):
    """the braces of the function whose definition starts with `head`"""
    i = text.index("{", text.index(head))
    depth, j = 1, i + 1
    while depth:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        j += 1
    return text[i:j]


def _where(pattern):
    return {f: len(re.findall(pattern, t)) for f, t in _sources().items() if re.search(pattern, t)}


def test_the_offsets_are_indexed_in_one_function():
    assert _where(r"cu\w*\[b \+ 1\]") == {"fa_device.h": 1}
    device = _code("fa_device.h")
    body = _function(device, "SeqRange seq_range(")
    assert "cu[b + 1]" in body and "cu[b]" in body and device.count("cu[b]") == 1
    # ... and the context length is clamped in one
    assert _where(r"max\(\w*(ctx|context_lens)\w*\[b\], 0\)") == {"fa_device.h": 1}
    assert "ctx[b]" in _function(device, "int seq_len(")
    # the five kernels that clamp call them (the bodies of the MLA kernels through MlaBlock); the backward kernels by the old name
    for f, calls in (("fa_fwd_paged_prefill_gfx950.hip", ("seq_len(p.ctx, b,", "seq_range(p.cu, b,")),
                     ("fa_merge_states_gfx950.hip", ("seq_len(p.ctx, b,", "seq_range(p.cu, b,")),
                     ("fa_mla_common.h", ("seq_len(p.ctx, b,", "seq_range_or_row(p.cu, b,")),
                     ("fa_mla_indexer_gfx950.hip", ("seq_len(p.ctx, b,", "seq_range_or_row(p.cu, b,")),
                     ("fa_varlen_common.h", ("seq_range(p.cu_q, b,", "seq_range(p.cu_k, b,")),
                     ("fa_bwd_varlen_gfx950.hip", ("seq_range(p.cu_k, b,",)), ("fa_bwd_mla_prefill_gfx950.hip", ("seq_range(p.cu_k, b,",))):
        for call in calls:
            assert call in _code(f), (f, call)
    assert _code("fa_mla_indexer_gfx950.hip").count("seq_range_or_row(") == 2      # the logits and the top-k kernel
    assert HAND_WRITTEN == {}


def test_the_block_lookup_is_written_once():
    assert _where(r"bs_shift >= 0 \?") == {"fa_device.h": 1}
    assert "bs_shift >= 0 ?" in _function(_code("fa_device.h"), "int block_of(")
    for f, n in (("fa_paged_tile.h", 1), ("fa_mla_common.h", 1), ("fa_mla_indexer_gfx950.hip", 2)):
        assert _code(f).count("block_of(") == n, f
    # the host's side of it: the power-of-two test
    assert _where(r"\(\w+ & \(\w+ - 1\)\) == 0") == {"fa_kernels.h": 1}
    assert "__builtin_ctz" in _function(_code("fa_kernels.h"), "inline int shift_of(")
    assert _where(r"bs_shift = ") == {f: 1 for f in ("fa_fwd_mla_paged_gfx950.hip", "fa_fwd_mla_sparse_gfx950.hip", "fa_fwd_paged_prefill_gfx950.hip",
                                                     "fa_fwd_paged_shared_prefix_gfx950.hip")} | {"fa_mla_indexer_gfx950.hip": 2}
    for f, t in _sources().items():
        for m in re.finditer(r"bs_shift = ([^;]+);", t):
            assert m.group(1) in ("shift_of(a.block_size)", "0"), (f, m.group(0))      # (0: the sparse call's flat cache, block size 1)


def test_the_length_cut_is_written_once():
    found = _where(r"max_seqlen(_[qk])? <(?!=)")
    assert found == {"fa_kernels.h": 1}, found
    assert "max_seqlen < total" in _function(_code("fa_kernels.h"), "inline int seqlen_cut(")
    capi = _code("aule_capi.cpp")
    assert capi.count("seqlen_cut(") == 8 and capi.count("cu_seqlens_q == nullptr ? 1 :") == 1
    assert "seqlen_cut(" in _function(capi, "static int max_sq_or_one(")


def test_the_split_plan_is_one_rule():
    # (the fp32 kernels' own split count, `n > tiles / 2`, is another rule: of dense fixed-length calls)
    found = _where(r"tiles / 2")
    assert found == {"fa_fwd_mla_paged_gfx950.hip": 2, "fa_fwd_f32.hip": 2, "fa_bwd_f32.hip": 2}, found
    assert _where(r"ns > tiles / 2") == {"fa_fwd_mla_paged_gfx950.hip": 1}
    dense, sparse = _code("fa_fwd_mla_paged_gfx950.hip"), _code("fa_fwd_mla_sparse_gfx950.hip")
    rule = _function(dense, "MlaPlan mla_split_plan(")
    assert "ns > tiles / 2" in rule and "kMlaMaxSplit" in rule and "device_cu_count(" in rule and "ws_bytes" in rule
    for text, head in ((dense, "MlaPlan mla_plan("), (sparse, "MlaPlan mla_sparse_plan(")):
        body = _function(text, head)
        assert "mla_split_plan(" in body and "ws_bytes" not in body and "device_cu_count" not in body, head
    assert "force_nsplit" in sparse and "force_nsplit" not in dense
    # one fill of the common parameters, one 16-bit dispatch
    common = _code("fa_mla_common.h")
    assert common.count("int mla_common_params(") == 1
    for text in (dense, sparse):
        assert text.count("mla_common_params(a, plan, ws, p)") == 1 and "p.part_ml =" not in text and "kLog2e" not in text
    assert _code("fa_device.h").count("int dispatch_16bit(") == 1
    for f in ("fa_fwd_mla_paged_gfx950.hip", "fa_fwd_mla_paged_fp8_gfx950.hip", "fa_fwd_mla_sparse_gfx950.hip", "fa_mla_indexer_gfx950.hip",
              "fa_merge_states_gfx950.hip"):
        t = _code(f)
        assert "dispatch_16bit(" in t and "kBF16" not in t and "kF16" not in t and "<Bf16Traits>" not in t, f


def test_the_c_api_states_its_shared_tails_once():
    capi = _code("aule_capi.cpp")
    assert capi.count("static int32_t dump_plan(") == 1 and capi.count("dump_plan({") == 5
    assert capi.count("& 0xffffffffull") == 1 and capi.count("ws_bytes >> 32") == 1      # the words of ws_bytes: dump_plan's alone
    assert capi.count("static int32_t mla_launch_tail(") == 1 and capi.count("return mla_launch_tail(d, plan, what,") == 2
    for name in ("mla_paged_launch", "mla_sparse_launch"):
        body = _function(capi, "static int32_t %s(" % name)
        assert "ScopedWorkspace" not in body and "DeviceGuard" not in body
        assert body.index("_desc_error(") < body.index("if (!initialised()) return -1;") < body.index("mla_launch_tail(")


def test_the_clamp_property_under_sanitizers(tmp_path):
    """Every combination of hostile offsets and lengths leaves [s, s + n) inside [0, T) and L inside [0, cap]: the helpers of fa_device.h
    compiled for the host with ASan + UBSan into a stand-alone program, which reads cu and ctx from exactly sized heap arrays."""
    line = makefile_compile_line()
    exe = tmp_path / "ragged_clamps"
    flags = [x for x in line[1:] if not x.startswith("-O")]
    r = subprocess.run([line[0]] + flags + ["-O1", "-g", "--cuda-host-only", "-x", "hip", "-Xarch_host", "-fsanitize=address,undefined",
                                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC, os.path.join(ROOT, "tests", "ragged_clamps_main.cpp"),
                                            "-fsanitize=address,undefined", "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert re.search(r"ok: (\d+) cases", r.stdout) and int(re.search(r"ok: (\d+) cases", r.stdout).group(1)) == 8 ** 3 * 3 * 3 * 2
