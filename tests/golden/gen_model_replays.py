"""Writes tests/golden/model_replays.json: what the host models of the match and of self-play compute on their fixtures — the
16-game fakenet match at every rule level (capture, king-safe, repetition, chase, chase off) greedy and with 6 sampled plies,
and the 16 whole self-play games with the chase rule, with it off, and at the repetition level.  Per replay the small per-game
arrays and a digest of the large one.  CPU only, about a minute.

    python tests/golden/gen_model_replays.py

The committed file was written before the models were unified, by the game loop that each rule level then had to itself, with
the nesting claims asserted (the chase loop with its switch off equalled the repetition loop, the repetition loop at fold 0 the
king-safe loop); this generator must reproduce it byte for byte from tests/test_model_replays_cpu.py's document()."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_model_replays_cpu as T   # noqa: E402


def main():
    doc = T.document()
    with open(os.path.join(HERE, "model_replays.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    for name, runs in doc["match"].items():
        print("  match %-10s reasons %s" % (name, {sp: sorted(set(r["reason"])) for sp, r in runs.items()}))
    for name, row in doc["selfplay"].items():
        print("  self-play %-9s %s" % (name, row["stats"]))


if __name__ == "__main__":
    main()
