"""Fixed-seed slices of tools/fuzz_serving.py inside the suite, as tests/test_gpu_fuzz.py holds those of tools/fuzz_parity.py: random valid
calls of the paged prefill (with the paged query and the paged decode where the batch is theirs), the paged cascade and
merge_attention_states, the paged MLA over 16-bit and FP8 latent caches, the varlen forward and backward, the three attention-sink entries
and the sink backward, the two tree-mask entries, and the MLA 192 / 128 prefill forward and backward -- every owned row of every draw
against the fp64 oracle through the judges of the hand-written files, plus the exact relations between the entries.  The seeds and
counts are tools/fuzz_serving.py's SLICES; tests/test_fuzz_serving_draws.py asserts, without a GPU, what these draws reach.  Deterministic:
a regression test over 150 configurations nobody enumerated by hand.  Each test prints the maxima it measured (pytest -s)."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fuzz(oracle_mod):   # (oracle_mod builds liboracle.so first; the tool imports `oracle` itself)
    spec = importlib.util.spec_from_file_location("fuzz_serving", os.path.join(_ROOT, "tools", "fuzz_serving.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _slice(fuzz, kind, count):
    n, seed = fuzz.SLICES[kind]
    assert n == count
    failures, worst = fuzz.run_slice(kind, n, seed)
    print("%s, %d draws at seed %d: maxima %s" % (kind, n, seed, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
    assert not failures, failures


def test_random_paged_prefill_batches(fuzz):
    """30 draws: rows and LSE vs the oracle, rows of no sequence never written, the Python entry equal to the C entry, and on uniform /
    all-decode batches the paged query and the paged decode"""
    _slice(fuzz, "prefill", 30)


def test_random_paged_cascade_batches(fuzz):
    """20 draws: rows and LSE vs the oracle over prefix plus own keys; P = 0 is the prefill; the prefill over the concatenated table;
    merge_attention_states of the prefix-only and own-keys states"""
    _slice(fuzz, "cascade", 20)


def test_random_paged_mla_batches(fuzz):
    """20 draws: decode and ragged, 16-bit and FP8 latent caches, one launch and key-range splits; two runs the same bits; FP8 with
    kv_scale = 1 the 16-bit call"""
    _slice(fuzz, "mla", 20)


def test_random_varlen_batches_forward_and_backward(fuzz):
    """20 draws: forward and backward through the C entries (strides, lead and tail rows, cuts by max_seqlen_*) and through the
    wrapper at padded head dims"""
    _slice(fuzz, "varlen", 20)


def test_random_attention_sink_calls(fuzz):
    """20 draws of the varlen (forward and backward, C entries into poisoned buffers, the wrapper at padded head dims), paged-prefill and
    paged-query sink entries: rows, LSE and gradients vs the fp64 judge of tests/test_gpu_sinks.py, dsinks within max(DSINKS_BAR, 4 x the
    error of a backward that reads O rounded to storage); heads with sink -inf the sinkless entry bit for bit; two runs the same bits;
    uniform batches through both paged kernels"""
    _slice(fuzz, "sinks", 20)


def test_random_tree_mask_calls(fuzz):
    """20 draws of the paged query tree and the paged prefill tree (C entry into poisoned out / lse): rows and LSE vs the judge of
    tests/test_gpu_tree.py under the drawn words; chain sequences and sequences of more than 64 tokens the plain entry bit for bit; two
    runs the same bits"""
    _slice(fuzz, "tree", 20)


def test_random_mla_prefill_batches_forward_and_backward(fuzz):
    """20 draws of aule_attention_mla_prefill_ex / _backward_ex in three memory layouts and of flash_attention_mla_varlen on slices of the
    projections: all six outputs vs the judge of tests/test_gpu_mla_backward.py; two runs the same bits; sequence 0 alone the same bits as in
    the batch"""
    _slice(fuzz, "mlapf", 20)
