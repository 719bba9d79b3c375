"""Fixed-seed slices of tools/fuzz_serving.py inside the suite, as tests/test_gpu_fuzz.py holds those of tools/fuzz_parity.py: random valid
calls of the paged prefill (with the paged query and the paged decode where the batch is theirs), the paged cascade and
merge_attention_states, the paged MLA over 16-bit and FP8 latent caches, the varlen forward and backward, the three attention-sink entries
and the sink backward, the two tree-mask entries, the MLA 192 / 128 prefill forward and backward, the sparse MLA, the MLA indexer (logits, top-k and the lists
through the sparse MLA) and the FP8-product paged prefill -- every owned row of every draw
against the fp64 oracle through the judges of the hand-written files, plus the exact relations between the entries.  The seeds and
counts are tools/fuzz_serving.py's SLICES; tests/test_fuzz_serving_draws.py asserts, without a GPU, what these draws reach.  Deterministic:
a regression test over 214 configurations nobody enumerated by hand.  Each test prints the maxima it measured (pytest -s)."""
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


def test_random_sparse_mla_calls(fuzz):
    """24 draws of aule_attention_mla_sparse_ex in the arena (0xFF outputs, guards, inputs unchanged, NaN bits in every unnamed cache row)
    and of flash_attention_mla_sparse: rows and LSE vs the judge of tests/test_gpu_mla_sparse.py over lists with invalid entries, whole
    invalid tiles and key ranges, repeated slots; one draw in three with a seam probe (a key 8 x q[t, h] at the ends of the list, the
    tiles and the key ranges; one probe head in two lists it twice) or an offset; the Python entry and two runs the same bits, forced
    key-range counts, contiguous lists equal to flash_attention_mla_paged bit for bit"""
    _slice(fuzz, "sparse", 24)


def test_random_mla_indexer_calls(fuzz):
    """20 draws of aule_mla_indexer_logits_ex / _topk_ex: every logit within the per-element bound of tests/test_gpu_mla_indexer.py, the
    Python entry and two runs the same bits, unit FP8 scales the 16-bit call; the top-k contract exactly on the kernel's own logits, the
    hand file's row kinds, ladders of last-place steps and random bit patterns; every selected key within two bounds of the k-th
    largest fp64 logit; one draw in four feeds the lists to the sparse MLA"""
    _slice(fuzz, "indexer", 20)


def test_random_paged_prefill_fp8mma_batches(fuzz):
    """20 draws of aule_attention_paged_prefill_fp8mma_ex into 0xFF-filled out / lse: LSE vs the q-rounded judge, out within atol + 2 E_P
    and the rms rule of tests/test_gpu_paged_prefill_fp8mma.py; zero, one-large-element and near-6e4 rows of q, spiked and offset keys
    through the cache's quantisation; the Python entry, two runs and sequence 0 alone the same bits; the plain entry on the same cache
    within its bound plus the distance between the two judges.  The LSE bound of a row is LSE_ATOL (hard draws: the fp32 rule) plus 2 E_acc,
    the accumulation of the FP8 matrix instruction (tools/fuzz_serving.py::fp8mma_acc_term): on the first slice the `big` and `near6e4` rows
    missed LSE_ATOL by 1.4 .. 3.0e-3 and 0.9 .. 2.1, and one-key rows showed the instruction itself 2^-12.4 of the largest product off."""
    _slice(fuzz, "fp8mma", 20)
