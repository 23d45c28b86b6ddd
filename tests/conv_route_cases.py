"""Reader of tests/golden/conv_routes.json (written by tools/record_conv_routes.py --merge): the recorded conv routes."""
import json
import os

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routes.json")


def load():
    """(fields, entries).  fields: the names of ppn_conv_desc in declaration order.  An entry: s (plan / train / layer / rejected /
    manual), d (the field values in that order, pointers as 0 / 1, splitk_ws 2 = misaligned; None: the NULL descriptor),
    k ([policy, ov_bp, ov_bc, conv64, strip]), rc, and error, or kernel, strip, stats_tiles (None: not asked) and cut."""
    with open(FIXTURE) as f:
        h = json.loads(f.readline())
        rows = [json.loads(line) for line in f]
    entries = []
    for r in rows:
        e = {"s": h["sources"][r[0]], "d": None, "k": h["knob_states"][r[3]], "rc": r[4]}
        if r[1] is not None:
            v = dict(zip(h["scalars"], r[2] + [0] * (len(h["scalars"]) - len(r[2]))))
            v.update({n: (r[1] >> i) & 1 for i, n in enumerate(h["pointers"])})
            if v["splitk_ws_misaligned"]:
                v["splitk_ws"] = 2
            e["d"] = [v[n] for n in h["fields"]]
        if r[4] != 0:
            e["error"] = r[5]
        else:
            e.update(kernel=h["kernels"][r[5]], strip=r[6], stats_tiles=None if r[7] < 0 else r[7], cut=r[8])
        entries.append(e)
    return h["fields"], entries
