"""DeepSeek-V3.2's lightning indexer: the step that makes the per-query token lists flash_mla_sparse_attn and
flash_mla_with_kvcache(..., indices=) attend over.  For query token t and cached token s

    I[t, s] = sum_h  w[t, h] * relu(q_I[t, h] . k_I[s])                    H_I = 32 or 64 index heads, 128 wide

and per query token the topk largest I[t, .] among the tokens it may see.  Three HIP launches (include/fa_mi355x.h: fa_indexer_pack,
fa_indexer_logits, fa_indexer_topk), each usable alone, and one wrapper that chains the last two:

    indexer_pack_cache(k_new, k_cache, cache_seqlens, block_table, *, scale_pow2=False)
    indexer_logits(q, weights, k_cache, cache_seqlens, block_table, *, causal=True, out=None, width=None) -> float32 (B, Nq, width)
    indexer_topk(logits, cache_seqlens, topk, *, seqlen_q=None, causal=True, out=None)                    -> int32 (B, Nq, topk)
    lightning_indexer(q, weights, k_cache, cache_seqlens, block_table, topk, *, causal=True)              -> int32 (B, Nq, topk)

The index-key cache k_cache is a paged pool (num_blocks, page_block_size, 1, W) of torch.uint8 or torch.float8_e4m3fn, the page size
a positive multiple of 16.  A cached token is 132 bytes, 128 e4m3 codes and one float32 scale at byte 128; its stride is >= 132 and a
multiple of 16 (W = 144 is the dense form; W = 132 views of a wider allocation keep their strides), and the bytes of a stride past
the 132 are never written and never read.  block_table int32 (B, max_blocks_per_seq) and cache_seqlens int32 (B,) (or an int) are
what the sparse attention calls take: one table serves both pools.  Both are untrusted: lengths are clamped on the device to
[0, min(max_blocks_per_seq * page_block_size, width)], no table entry past ceil(len / page) is read, a page outside the pool is not
fetched (the logits read it as a zero key with scale 0, logit 0; the append drops the token).  Nothing is read on the host, nothing
synchronises: every call can be captured in a graph and replayed after lengths, table, cache bytes and weights changed in place.

Visibility, as for flash_mla_sparse_attn: key j of sequence b is visible to token i iff 0 <= j < len_b and, if causal,
j <= len_b - Nq + i; len_b = cache_seqlens[b] counts the Nq new tokens (append first).

q is (B, Nq, H_I, 128) torch.float8_e4m3fn (the caller quantises it), weights (B, Nq, H_I) float32 with the query's own scale and
the H_I^-1/2 d^-1/2 factors folded in, as the model does.  indexer_logits writes ONLY the visible entries of its result; the rest of
a fresh result is uninitialised memory, and indexer_topk never reads it.

indexer_topk's result is fully specified: with key(x) = bits(x) ^ (sign ? 0xFFFFFFFF : 0x80000000) compared as unsigned (-0 < +0, a
positive NaN above +inf), a row's selected set is its min(topk, n) visible positions largest by (key descending, position
ascending), written in ascending position order and followed by -1.  A pure function of the logits' bits.

Refusals, before anything runs: a 16-bit or other-float8 q, widths other than 128, head counts other than 32 / 64, lengths or a table
that are not int32 raise NotImplementedError with the argument's name; wrong shapes and devices RuntimeError.  No gradient, no CPU
path."""
from __future__ import annotations

import torch

__all__ = ["indexer_pack_cache", "indexer_logits", "indexer_topk", "lightning_indexer"]


def _detached(t):
    return t.detach() if isinstance(t, torch.Tensor) else t


def indexer_pack_cache(k_new, k_cache, cache_seqlens, block_table, *, scale_pow2=False):
    """Quantise new index keys and append them to the pool, in place.  k_new (B, N_new, 128) bfloat16; token i of sequence b goes to
    position cache_seqlens[b] + i (the lengths before the append; not modified).  In fp32 from the exact bfloat16 values:
    scale = amax / 448 (1 for an all-zero row; scale_pow2: rounded up to a power of two), byte = e4m3(clamp(x / scale, +-448)),
    round to nearest even: mla_fp8_pack_cache's rule on one 128-wide tile.  Returns None."""
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        ext.ex_indexer_pack(_detached(k_new), k_cache, cache_seqlens, block_table, bool(scale_pow2))


def indexer_logits(q, weights, k_cache, cache_seqlens, block_table, *, causal=True, out=None, width=None):
    """float32 (B, Nq, width) index logits, width = max_blocks_per_seq * page_block_size by default;
    logits[b, i, j] = (sum_h w[b, i, h] * max(0, q[b, i, h] . k8[j])) * k_scale[j] for every visible key j, the products on the
    e4m3 matrix instruction and the rest in fp32.  Entries that are not visible are not written (out keeps its bytes there)."""
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        return ext.ex_indexer_logits(_detached(q), _detached(weights), k_cache, cache_seqlens, block_table, bool(causal), out, width)


def indexer_topk(logits, cache_seqlens, topk, *, seqlen_q=None, causal=True, out=None):
    """int32 (B, Nq, topk): per row the selected positions in ascending order, then -1 (module docstring).  logits float32
    (B, Nq, width) from any source; seqlen_q, if given, must be Nq.  With no more visible keys than topk the logits are not read."""
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        return ext.ex_indexer_topk(_detached(logits), cache_seqlens, topk, seqlen_q, bool(causal), out)


def lightning_indexer(q, weights, k_cache, cache_seqlens, block_table, topk, *, causal=True):
    """indexer_topk(indexer_logits(...), ...) to the bit, the logits kept in the library's persistent workspace: after the first
    call of a shape only the result is allocated."""
    import flashattention_lab_cuda as ext

    with torch.no_grad():
        return ext.ex_lightning_indexer(_detached(q), _detached(weights), k_cache, cache_seqlens, block_table, topk, bool(causal))
