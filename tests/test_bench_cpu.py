"""bench.py host logic without a GPU: defaults of the measurement flags, the two-stream
region's memory check (no device -> no second batch), and the step functions."""
import bench
import tkz
from tkz import synth


def test_bench_defaults():
    a = bench.parse_args([])
    assert a.gpus == 1 and a.config == 1 and a.streams == 1
    assert not a.no_pipelined_run and not a.no_memo_off_run and not a.no_cpu_baseline
    assert not a.full and a.dump_outputs == ""


def test_plain_run_times_the_primary_region_only():
    """Without --full every other region, the verification and the CPU baseline are off;
    --full leaves the flags as given."""
    a = bench.plain_run(bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"]))
    assert (a.steps, a.warmup) == (7, 2)
    assert a.no_verify and a.no_memo_off_run and a.no_pipelined_run and a.no_cpu_baseline
    assert a.no_host_e2e and a.no_single_doc and a.no_decode_pad and bench.secondary_regions(a) == []
    f = bench.plain_run(bench.parse_args(["--full", "--no-host-e2e"]))
    assert f.no_host_e2e and not (f.no_verify or f.no_memo_off_run or f.no_pipelined_run or f.no_cpu_baseline or
                                  f.no_single_doc or f.no_decode_pad)
    assert bench.secondary_regions(f) == bench.SECONDARY


def test_two_batches_fit_without_device():
    """tkz_dev_mem_info fails without a GPU: the pipelined region is skipped, not guessed."""
    tok = tkz.Tokenizer.from_json(synth.tokenizer_json(0))
    assert bench.two_batches_fit(tok, 1 << 20, 1000) is False


def test_stream_steps_single_batch():
    """One batch runs on the tokenizer's own stream (no HIP stream is created)."""

    class FakeBatch:
        def __init__(self):
            self.runs = self.syncs = 0

        def run(self, stream=None):
            self.runs += 1

        def sync(self):
            self.syncs += 1

    b = FakeBatch()
    step, sync = bench.stream_steps(tkz, [b])
    step(), step(), sync()
    assert (b.runs, b.syncs) == (2, 1)
