#!/usr/bin/env python3
"""Record tests/golden/device_flash_{f32,q28}.json from the firmware build of the oracle (oracle/_ref/libref_fw_*): the scripted request
sequence of tests/flash_script.py, the firmware's answer to every step, and what a host reads back at the end (every GET request, the
parameter blob, a collected slot image, the 48 KB flash).  tests/test_device_flash_cpu.py::test_replay_recorded_fixture replays it on the
library, so a machine without the firmware build still holds dspi_device_flash to the reference's recorded behaviour.

    python tools/gen_flash_fixture.py        (needs oracle/_ref; rewrites both files)"""
import base64
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import flash_script as FS      # noqa: E402
from orclib import Oracle      # noqa: E402


def main():
    enc = lambda r: r.hex() if isinstance(r, bytes) else r
    for flavor in (1, 0):
        fw = Oracle(flavor, ref="fw")
        dev = FS.FwDev(fw)
        steps = FS.scripted(flavor)
        answers = [enc(FS.apply(dev, s)) for s in steps]
        end = FS.observe(dev)
        fx = dict(flavor=flavor, steps=steps, answers=answers, probes=[list(p) for p in FS.PROBES], gets=[enc(g) for g in end["gets"]],
                  bulk=end["bulk"].hex(), slot=end["slot"].hex(), flash=base64.b64encode(zlib.compress(end["flash"], 9)).decode())
        path = os.path.join(ROOT, "tests", "golden", f"device_flash_{'f32' if flavor else 'q28'}.json")
        with open(path, "w") as f: json.dump(fx, f, separators=(",", ":"))
        print(path, os.path.getsize(path), "bytes,", len(steps), "steps")
        fw.close()


if __name__ == "__main__":
    main()
