#!/usr/bin/env python3
"""What every form of the partitioned substep reports of its exchanges (hns_dist_info: exchanges, messages, packed exchanges, bytes per region type) after one core and
one full substep -- tests/dist_cases.py: EXCHANGE_FORMS --, and what the ranks of the smallest multi-process case (plume, 3 processes, k = 2) report after its two
core substeps. Run on the build whose figures are to be the record (HNS_LIBRARY = the parent commit's library when a change must issue the same exchanges):

    HNS_LIBRARY=<parent's libhns.so> python profiles/micro/dist_exchange_counts.py tests/golden/dist_exchange_counts.json

tests/test_dist_gpu.py compares what the build under test reports with that file for equality. Starts 3 processes."""
import json
import os
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dist_cases  # noqa: E402
import test_dist_gpu  # noqa: E402

record = {form: dist_cases.exchange_counts(form) for form in dist_cases.EXCHANGE_FORMS}
with tempfile.TemporaryDirectory() as tmp:
    got = test_dist_gpu._run_processes(3, "plume", 2, 7, 2, tmp)
    record["ipc_plume_3_k2"] = [{"exchanges": int(g["exchanges"]), "messages_sent": int(g["messages"])} for g in got]
text = json.dumps(record, indent=None, separators=(",", ":"), sort_keys=True)
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(text + "\n")
