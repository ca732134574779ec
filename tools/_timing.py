"""What the tools/*_time.py share: HIP-event timing of a call and the ``--json FILE`` tail."""
import json
import sys

import torch


def timed(fn, warmup=5, calls=20):
    """(the last result of ``fn()``, the HIP-event times [ms] of ``calls`` calls after ``warmup`` untimed ones)"""
    times, out = [], None
    for it in range(warmup + calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            times.append(e0.elapsed_time(e1))
    return out, times


def write_json(results, **extra):
    """with ``--json FILE`` on the command line: the device's name, ``extra`` and the result rows into FILE"""
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), **extra, results=results), fh, indent=1)
