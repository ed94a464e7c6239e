#!/usr/bin/env python
"""The parity log (the parity_errors.jsonl that tests/parity_log.py appends to: the lines of tests/test_gpu_learner_edges.py) ->
profiles/learner_edges_parity_errors.json:
per case and run (variant0 / default / pipelined) the maximum over its updates of every tensor's error / scale (the bar of every
figure is 1e-5: tests/learner_edge_cases.py; 'params:*' in units of atol + rtol |want|, scaled to the same bar), the updates with
an ambiguous ReLU gate apart (judged at 100x), the smallest ReLU margin, and the maxima over all cases.

    python tools/learner_edges_summary.py PARITY_LOG > profiles/learner_edges_parity_errors.json"""
import json
import re
import sys


def main():
    cases, worst = {}, {}
    for line in open(sys.argv[1]):
        line = line.strip()
        if not line.startswith('{"case": "learner_edges['):
            continue
        r = json.loads(line)
        m = re.match(r"learner_edges\[(\S+) (\S+)\] (update \d+|actor at slot \d+)( \(ambiguous ReLU gate\))?$", r.pop("case"))
        name, run, what, ambiguous = m.groups()
        c = cases.setdefault(name, {}).setdefault(run, {"updates": 0, "ambiguous_updates": [], "max": {}, "max_ambiguous": {}})
        margin = r.pop("relu_margin", None)
        if what.startswith("update"):
            c["updates"] += 1
            c["min_relu_margin"] = min(c.get("min_relu_margin", 1e9), margin)
            if ambiguous:
                c["ambiguous_updates"].append(int(what.split()[1]))
        into = c["max_ambiguous"] if ambiguous else c["max"]
        for k, v in r.items():
            into[k] = max(into.get(k, 0.0), v)
            if not ambiguous:
                kind = k.split(":")[0]
                if v > worst.get(kind, (0.0,))[0]:
                    worst[kind] = (v, "%s %s %s: %s" % (name, run, what, k))
    for runs in cases.values():
        for c in runs.values():
            if not c["max_ambiguous"]:
                del c["max_ambiguous"]
    print(json.dumps({"what": "error / scale of every tensor the learner edge suite compares with its float64 reference, per case and "
                              "run: the maximum over the case's updates (bar 1e-5 each; updates with a ReLU input within 5e-7 of zero "
                              "apart, judged at 100x)",
                      "largest": {k: {"figure": v, "where": w} for k, (v, w) in sorted(worst.items())}, "cases": cases}, indent=1))


if __name__ == "__main__":
    main()
