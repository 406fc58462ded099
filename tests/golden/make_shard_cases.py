"""Regenerates tests/golden/shard_cases.json: the pins of the block and sharded entry points' cases (tests/shardgen.py).

    python tests/golden/make_shard_cases.py

No input byte and no stream byte is stored: names, sizes, digests of the inputs and of the expected outputs, the wanted codes and
the number of cases each GPU test has to run."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import shardgen  # noqa: E402
from oracle.pyoracle import Oracle, build  # noqa: E402

if __name__ == "__main__":
    build()
    pins = shardgen.pins(Oracle())
    with open(os.path.join(HERE, "shard_cases.json"), "w") as f:
        json.dump(pins, f, indent=1, sort_keys=True)
        f.write("\n")
    print({k: len(v) for k, v in pins.items()}, pins["counts"])
