"""Shared by test_gpu_parity.py and test_gpu_shape_modes.py: the strict build's bar against the oracle, and the log of measured parity figures."""


def report(rec):
    """Append one JSON line of measured parity figures to gpurun_out/parity_report.jsonl (copied to profiles/)."""
    import json
    import os
    from conftest import ROOT
    d = os.path.join(ROOT, "gpurun_out")
    if os.path.isdir(d):
        with open(os.path.join(d, "parity_report.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")


def check_exact(got, want, what="", allow=0):
    """The strict build's bar: every pixel equal.  (At the multi-megapixel sizes a handful of pixels differ where the device libm and the
    oracle's glibc round one sinf / cosf / powf value differently: those frames go through pin_strict_residual instead.)"""
    bad = int((got != want).sum())
    report(dict(test=what, pixels=int(got.size), differing=bad, allowed=allow))
    assert got.shape == want.shape and bad <= allow, f"{what}: {bad} of {got.size} pixels differ from the oracle (allowed {allow})"
