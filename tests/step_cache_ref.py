"""Torch restatement of the first-block step cache (include/bya.h "First-block step cache"): the three
kernels as plain tensor arithmetic -- fp32 differences of bf16 values rounded to bf16 by torch (round to nearest even), the
probe's two sums in fp64 from EXACT differences (a difference of two bf16 values is exact in fp64) -- and the policy.  Runs on
whatever device its tensors are on; the tests keep it on the CPU."""
import math

import torch


def bf16_rne(f):
    """fp32 -> bf16, round to nearest even; every NaN becomes the quiet NaN 0x7fc0 (torch's own converters disagree on a
    NaN's bits -- 0x7fc0 from the scalar path, 0xffff from the vectorised one --, the definition takes the first)."""
    nan = torch.tensor([0x7FC0], dtype=torch.int16, device=f.device).view(torch.bfloat16)
    return torch.where(f.isnan(), nan, f.to(torch.bfloat16))


def bf16_sub(a, b):
    """bf16_rne(float(a) - float(b))"""
    return bf16_rne(a.float() - b.float())


def probe(x, E, r_ref):
    """-> (r_new, the new E, num, den): r_new = bf16(x - E); E <- x; num = sum |r_new - r_ref|, den = sum |r_ref| in fp64
    (r_new as stored, i.e. rounded); both 0.0 where ``r_ref`` is None."""
    r_new = bf16_sub(x, E)
    if r_ref is None:
        return r_new, x.clone(), 0.0, 0.0
    num = (r_new.double() - r_ref.double()).abs().sum().item()
    den = r_ref.double().abs().sum().item()
    return r_new, x.clone(), num, den


def capture(x, E):
    """R = bf16(x - E)"""
    return bf16_sub(x, E)


def apply(x, R):
    """bf16(x + R)"""
    return bf16_rne(x.float() + R.float())


def distance(num, den):
    if math.isnan(num) or math.isnan(den):
        return math.nan
    return math.inf if den == 0.0 else num / den


def decide(num, den, has_ref, hits, threshold, max_hits):
    """Re-use if and only if a reference exists, d < threshold and hits < max_hits (None: unbounded); NaN compares false."""
    d = distance(num, den)
    return bool(has_ref and d < threshold and (max_hits is None or hits < max_hits))


def pattern(distances_ok, max_hits):
    """The F / R pattern of a run whose every comparison passes (``distances_ok`` steps behind the first): for the tests of
    the hit cap."""
    out, hits, has_ref = [], 0, False
    for _ in range(distances_ok):
        r = decide(0.0, 1.0, has_ref, hits, math.inf, max_hits)
        out.append("R" if r else "F")
        hits = hits + 1 if r else 0
        has_ref = True
    return "".join(out)
