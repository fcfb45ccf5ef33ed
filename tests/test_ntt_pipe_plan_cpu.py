"""The decision of the transform's launcher between the caller's stream alone and the pipelined chunk schedule
(moai_ntt_pipe_plan, the host function csrc/ntt.hip ntt_launch itself calls): chunks on the busiest side stream, 0 for the
single-stream form.  Host arithmetic only, no GPU."""
import pytest

N16, L44 = 1 << 16, 44
POLY = L44 * N16 * 8  # 22 MiB: one polynomial of the bench's workload


def test_no_schedule_without_streams_chunks_or_work(moai):
    plan = moai.hip.ntt_pipe_plan
    assert plan(512, L44, N16, 4 * POLY, 0) == 0    # MOAI_NTT_PIPE=0
    assert plan(512, L44, N16, 4 * POLY, -1) == 0
    assert plan(512, L44, N16, 0, 3) == 0           # no chunk size: one chunk
    assert plan(0, L44, N16, POLY, 3) == 0
    assert plan(512, 0, N16, POLY, 3) == 0
    assert plan(512, L44, 0, POLY, 3) == 0


def test_threshold_is_two_chunks(moai):
    plan = moai.hip.ntt_pipe_plan
    assert plan(1, L44, N16, POLY, 3) == 0          # a single polynomial is a single chunk
    assert plan(4, L44, N16, 4 * POLY, 2) == 0      # the batch is one chunk
    assert plan(4, L44, N16, 400 * POLY, 2) == 0    # a chunk larger than the batch
    assert plan(5, L44, N16, 4 * POLY, 2) == 1      # 4 + 1 polynomials, one chunk per stream
    assert plan(2, L44, N16, POLY, 1) == 2          # one side stream: the chunk loop, off the caller's stream


def test_chunks_are_whole_polynomials_and_at_least_one(moai):
    plan = moai.hip.ntt_pipe_plan
    assert plan(512, L44, N16, POLY, 1) == 512
    assert plan(512, L44, N16, POLY - 1, 1) == 512      # smaller than a polynomial: one polynomial
    assert plan(512, L44, N16, 1, 1) == 512
    assert plan(512, L44, N16, 2 * POLY - 1, 1) == 512  # rounded down
    assert plan(512, L44, N16, 2 * POLY, 1) == 256
    assert plan(511, L44, N16, 2 * POLY, 1) == 256      # a short last chunk counts
    assert plan(6, 1 << 40, 1 << 40, 1 << 30, 2) == 3   # a polynomial beyond size_t is beyond any chunk


def test_streams_are_capped_at_three_and_at_the_chunks(moai):
    plan = moai.hip.ntt_pipe_plan
    assert plan(512, L44, N16, 4 * POLY, 2) == 64
    assert plan(512, L44, N16, 4 * POLY, 3) == 43       # 128 chunks: 43 + 43 + 42
    assert plan(512, L44, N16, 4 * POLY, 4) == 43       # never more than three side streams
    assert plan(512, L44, N16, 4 * POLY, 1 << 40) == 43
    assert plan(2, L44, N16, POLY, 3) == 1              # two chunks use two streams
    assert plan(5, 3, 4096, 3 * 4096 * 8, 3) == 2       # 2 + 2 + 1: one stream with a single chunk
    assert plan(5, 3, 4096, 2 * 3 * 4096 * 8, 2) == 2   # chunks of 2 + 2 + 1 polynomials on two streams


def test_small_batches_stay_on_the_callers_stream(moai):
    plan = moai.hip.ntt_pipe_plan
    assert plan(512, L44, N16, 4 * POLY, 2, 64) == 64   # 128 chunks on two streams: exactly the minimum
    assert plan(512, L44, N16, 4 * POLY, 2, 65) == 0
    assert plan(508, L44, N16, 4 * POLY, 2, 64) == 64   # 127 chunks: 64 + 63, the busiest stream counts
    assert plan(504, L44, N16, 4 * POLY, 2, 64) == 0    # 126 chunks: 63 + 63
    assert plan(512, L44, N16, 4 * POLY, 3, 43) == 43
    assert plan(512, L44, N16, 4 * POLY, 3, 44) == 0
    assert plan(5, 3, 4096, 3 * 4096 * 8, 3, 0) == 2    # no minimum
    assert plan(5, 3, 4096, 3 * 4096 * 8, 3, -7) == 2
    assert plan(5, 3, 4096, 3 * 4096 * 8, 3, 3) == 0
