"""Shared inputs of the cz_search_lines tests (TEST INFRASTRUCTURE): the corpus positions tests/test_hip_search.py::
test_search_vs_oracle_batch picks, and a lock-step driver that runs any engine with the host-array interface of
tests/searchdrive.py (the C oracle's Search, or an adapter around the HIP SearchEngine) under a fakenet forward."""
import numpy as np


def corpus(rules_golden, n):
    """The first n of rules.npz's positions with both kings and a move, every 11th -> (boards [n, 90], side [n], rr [n] = 0)."""
    g = rules_golden
    ok = [(g["boards"][i] == 1).any() and (g["boards"][i] == 8).any() and g["counts"][i] > 0 for i in range(len(g["boards"]))]
    idx = np.nonzero(ok)[0][::11][:n]
    assert len(idx) == n
    return g["boards"][idx].copy(), g["side"][idx].astype(np.uint8), np.zeros(n, np.int32)


def run_ply(engine, forward, playouts):
    """The root expansion and `playouts` lock-steps on every tree of `engine`."""
    for step in range(1 + playouts):
        planes, _ = engine.select(0 if step == 0 else 1)
        logits, value = forward(planes)
        engine.expand_backup(logits, value)


def greedy(stats):
    """The most visited root child of every tree (first maximum, generation order), 0xFFFF for a root without children."""
    G = len(stats["count"])
    played = np.full(G, 0xFFFF, np.uint16)
    for g in range(G):
        n = int(stats["count"][g])
        if n:
            played[g] = stats["label"][g, int(np.argmax(stats["N"][g, :n]))]
    return played
