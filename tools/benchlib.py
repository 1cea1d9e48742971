"""What the tools/bench_*.py measurements share: the timing procedure, the command line, and the process set-up.

    from benchlib import arm, parser, quiet, timed_ms      (python tools/bench_X.py puts tools/ on sys.path itself)

Importing it puts the repository root, tests/golden (synth) and tests (the *_ref modules) on sys.path."""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import signal
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed_ms(fn, iters, warmup, repeats):
    """(median, min, max) over `repeats` blocks of `iters` calls (device events around each block), per call, after `warmup`
    calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


def rounded_ms(fn, iters, warmup, repeats):
    """timed_ms as the list [median, min, max] rounded to 4 places: the three values of a `name`, `name_min`, `name_max` key."""
    return [round(v, 4) for v in timed_ms(fn, iters, warmup, repeats)]


def quiet(fn, *a, **k):
    """fn(*a, **k) with stdout swallowed (the models print their shapes when constructed)."""
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def parser(doc, repeats=5, iters=20, warmup=3, limit=540):
    """The --repeats / --iters / --warmup / --limit command line of a bench tool, described by its docstring's first paragraph."""
    ap = argparse.ArgumentParser(description=doc.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=repeats)
    ap.add_argument("--iters", type=int, default=iters)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--limit", type=int, default=limit, help="seconds after which the process ends itself")
    return ap


def arm(tool, limit):
    """Exits where there is no GPU; otherwise the process ends itself after `limit` seconds (SIGALRM)."""
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool} needs an MI355X: there is no CPU fallback and no CPU timing")
    signal.alarm(limit)
