"""Regenerates tests/golden/encoder_catalogue.json: the pins of the encoder catalogue (tests/encgen.py).

    python tests/golden/make_encoder_catalogue.py

Run it where oracle/_ref/libtsq_ref.so is built: every stream is compared with the compiled reference's before it is pinned and the
entry records "reference_checked": true.  No input byte and no stream byte is stored: digests, lengths and the census only."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import encgen  # noqa: E402
from oracle.pyoracle import Oracle, Reference, build  # noqa: E402

if __name__ == "__main__":
    build()
    ref = Reference() if Reference.available() else None
    if ref is None:
        print("warning: no compiled reference here; the entries will say reference_checked: false")
    pins = encgen.pins(Oracle(), ref)
    with open(os.path.join(HERE, "encoder_catalogue.json"), "w") as f:
        json.dump(pins, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(pins), "cases pinned; reference checked:", all(e["reference_checked"] for e in pins.values()))
