"""What the reference's own programs (oracle/_ref: rmfmt, rm2ct, rmprune, efn_drv, efn2_drv, dbutil_drv, built
from the reference's sources by oracle/Makefile) print for the inputs of the tests, pinned in
tests/golden/ref_pins.json -- energies as numbers, longer outputs as md5 sums -- so that those tests run
without the reference.  RNAMOTIF_PIN_REF=1 (with oracle/_ref built) runs the programs again and rewrites the pins."""
import hashlib
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
PATH = os.path.join(ROOT, "tests", "golden", "ref_pins.json")
RECORD = os.environ.get("RNAMOTIF_PIN_REF") == "1"

_pins = None


def md5(data: bytes) -> str:
    return hashlib.md5(data).hexdigest()


def pinned(key: str, make):
    """The pin `key`; when recording, make() -- which runs the reference's program -- gives it afresh."""
    global _pins
    if _pins is None:
        _pins = json.load(open(PATH)) if os.path.exists(PATH) else {}
    if RECORD:
        assert os.path.isdir(REF), "RNAMOTIF_PIN_REF=1 needs oracle/_ref (oracle/Makefile, target ref)"
        _pins[key] = json.loads(json.dumps(make()))
        with open(PATH, "w") as f:
            json.dump(_pins, f, indent=0, sort_keys=True)
            f.write("\n")
    assert key in _pins, "no pin %r in tests/golden/ref_pins.json (RNAMOTIF_PIN_REF=1 with oracle/_ref built records it)" % key
    return _pins[key]
