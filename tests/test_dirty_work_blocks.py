"""Every device entry point on a caller's work block that holds arbitrary bytes (the product library; no switch involved).

A caller's work block is a recycled buffer: under PyTorch a tensor the allocator has handed out before.  The fifteen `*_device`
entry points promise that what they compute does not depend on its contents, and tests/test_streams.py fills it with the one
word that is legal in every table.  Here every entry point and every variant of `test_streams.CASES` runs on the null stream
with the block filled with each of zero, small (words in 0 .. 4), 0xA5, 0xFF and random words: the outputs and their canaries
must equal the CPU reference bit for bit, the host value too, and the statistics getters must read what the unfilled
null-stream call reports.  A slab that is one word short, a counter cleared one stage late or a flag array zeroed for n entries
and read for n + 1 gives another answer under at least one of them.

The entry points that read their text or query by words (build, LCP, match, score, substrings) are run again with the 16 slack
bytes behind every input set to 0xFF and to 0x00: the answers must not move.

Cases, buffers, comparison and the null-stream baseline are test_streams' own, imported."""
import numpy as np
import pytest

import dirty_blocks
from test_streams import CASES, EVERY, Buffers, compare, env, null_stream_stats      # noqa: F401 -- env is the module's fixture

D2H, D2D = 2, 3
WORD_READERS = ("sa_amd_saca_device", "sa_amd_lcp_device", "sa_amd_index_match_stats_device", "sa_amd_index_match_spans_device",
                "sa_amd_index_infgram_score_device", "sa_amd_substrings_device")
SLACK = [pytest.param(fn, v, id=fn[len("sa_amd_"):] + "-" + v.name) for fn in WORD_READERS for v in CASES[fn]]


def run_on_null_stream(env, v, pattern=None, slack=None):
    """one call on the null stream: the work block overwritten with `pattern` (None: test_streams' ones), the 16 bytes behind
    every input with `slack`; outputs, canaries, host value and statistics as the module docstring says"""
    want_stats = null_stream_stats(env, v)
    hip = env.hip
    b = Buffers(env, v, None if pattern is None else (lambda size: dirty_blocks.fill_bytes(pattern, size, seed=len(v.name))))
    try:
        b.load("real")
        if b.wb:
            assert hip.hipMemcpy(b.work, b.fill, b.wb, D2D) == 0
        if slack is not None:
            for p, size in zip(b.ins, b.sizes):
                assert hip.hipMemset(p + size, slack, 16) == 0
        assert hip.hipDeviceSynchronize() == 0
        host = b.call(0)
        stats = v.stats()
        raw = [np.zeros(s + 512, dtype=np.uint8) for s in b.out_sizes]
        for p, r in zip(b.outs, raw):
            assert hip.hipMemcpy(r.ctypes.data, p, r.size, D2H) == 0
        compare(v, raw, host, where=f"work block {pattern}, slack {slack}")
        assert stats == want_stats, (v.name, pattern, slack, stats, want_stats)
    finally:
        b.free()


def test_every_entry_point_that_reads_by_words_is_a_case():
    assert set(WORD_READERS) <= set(CASES) and len(SLACK) >= len(WORD_READERS)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", dirty_blocks.ORDER)
@pytest.mark.parametrize("fn,v", EVERY)
def test_entry_point_on_a_dirty_work_block(env, fn, v, pattern):
    run_on_null_stream(env, v, pattern=pattern)


@pytest.mark.gpu
@pytest.mark.parametrize("slack", [0xFF, 0x00], ids=["ff", "00"])
@pytest.mark.parametrize("fn,v", SLACK)
def test_entry_point_with_dirty_slack_behind_its_inputs(env, fn, v, slack):
    run_on_null_stream(env, v, slack=slack)
