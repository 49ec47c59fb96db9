"""Pure-Python reference of the K8 latency chain (``csrc/probe/chase_latency.h``): no GPU, no native code.

The chain has ``n`` nodes, ``n`` a power of two; node ``i`` points at ``next(i) = (A*i + C) mod n``.
``C`` is odd and ``A = 1 (mod 4)``, so by the Hull-Dobell theorem the map is a single cycle through all
``n`` nodes.  ``chain_skip`` composes the affine map by doubling, so the node any number of hops away
costs O(log hops); the host driver uses the same closed form to check where every lane ends.
"""
from __future__ import annotations

from typing import List, Tuple

__all__ = ["CHAIN_A", "CHAIN_C", "chain_next", "chain_skip", "chain_starts"]

CHAIN_A = 1664525
CHAIN_C = 1013904223


def _check_n(n: int) -> None:
    if n < 2 or n & (n - 1):
        raise ValueError(f"n must be a power of two >= 2, got {n}")


def chain_next(i: int, n: int) -> int:
    """The successor of node ``i`` in a chain of ``n`` nodes."""
    _check_n(n)
    return (CHAIN_A * i + CHAIN_C) % n


def _power(hops: int, n: int) -> Tuple[int, int]:
    """(a, c) with next^hops(x) = (a*x + c) mod n."""
    ra, rc = 1, 0
    fa, fc = CHAIN_A % n, CHAIN_C % n
    while hops:
        if hops & 1:
            ra, rc = (fa * ra) % n, (fa * rc + fc) % n
        fa, fc = (fa * fa) % n, (fa * fc + fc) % n
        hops >>= 1
    return ra, rc


def chain_skip(start: int, hops: int, n: int) -> int:
    """The node reached from ``start`` after ``hops`` hops, in O(log hops)."""
    _check_n(n)
    if hops < 0:
        raise ValueError("hops >= 0")
    a, c = _power(int(hops), n)
    return (a * start + c) % n


def chain_starts(n: int, chains: int) -> List[int]:
    """Where lane ``l`` of ``chains`` starts: ``(l * n) // chains`` hops from node 0, so the lanes are
    spread evenly over the cycle."""
    _check_n(n)
    if chains < 1:
        raise ValueError("chains >= 1")
    return [chain_skip(0, (l * n) // chains, n) for l in range(chains)]
