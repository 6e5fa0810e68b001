"""What the bench_*.py tools of the native ops share: the GPU guard, alternating timed steps, the launch count of a step, the
JSON-lines epilogue.  Each tool keeps its baseline formulation, its cases and what it derives from the timings."""
import json
import os

import torch


def require_gpu(who):
    """-> cuda:0, or the tool ends: a CPU timing would mean nothing"""
    if not torch.cuda.is_available():
        raise SystemExit('%s: needs the GPU (no CPU timing is meaningful)' % who)
    return torch.device('cuda:0')


def summary(times):
    ts = sorted(times)
    return {'median_ms': ts[len(ts) // 2], 'p10_ms': ts[len(ts) // 10], 'p90_ms': ts[(len(ts) * 9) // 10]}


def time_alternating(steps, iters, warmup):
    """steps: name -> callable, in the order they take turns.  Every step is warmed up; then `iters` rounds, each call inside its
    own pair of device events on the current stream.  -> name -> median / 10th / 90th percentile in ms"""
    for _ in range(warmup):
        for f in steps.values():
            f()
    torch.cuda.synchronize()
    times = {name: [] for name in steps}
    for _ in range(iters):
        for name, f in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    return {name: summary(ts) for name, ts in times.items()}


def count_launches(step, who, required=False):
    """Device kernels and copies of one step, by torch.profiler.  A count the profiler cannot give is None and a printed line,
    or an error for a tool whose claim is the count (required)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
    except Exception as e:
        if required:
            raise
        print('%s: launches not counted (%s)' % (who, e), flush=True)
        return None
    if n == 0 and required:
        raise RuntimeError('%s: torch.profiler reported no device activity for a step' % who)
    return n or None


def emit(results, out, echo=True):
    """One JSON line per result: into the file `out` if given, and printed unless the tool has printed them as it went"""
    lines = [json.dumps(r) for r in results]
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    if echo:
        for line in lines:
            print(line, flush=True)
