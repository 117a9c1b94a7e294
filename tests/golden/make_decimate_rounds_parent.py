"""Record what the device decimation rounds return, as digests, for tests/test_gpu_decimate_golden.py:
run with the library the later builds are to be compared with (needs a GPU), from the repository root:

    python tests/golden/make_decimate_rounds_parent.py

Writes tests/golden/decimate_rounds_parent.json and decimate_rounds_parent_large.json and refuses to
overwrite either (an existing one is left as it is): the record is of one library, taken once,
before the kernels it pins are changed."""
import json
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
from tests.test_decimate_rounds_host import MESHES, decimation_meshes  # noqa: E402
from tests.test_gpu_decimate_golden import (GOLDEN, GOLDEN_LARGE, MAX_ROUNDS, case_key, large_case, run_case,  # noqa: E402
                                            workspace_cases)


def main():
    dev = torch.device("cuda:0")
    if os.path.exists(GOLDEN_LARGE):
        print("%s exists: not overwritten" % GOLDEN_LARGE)
    else:
        rec = large_case(dev)
        assert rec == large_case(dev), "two runs differ"
        with open(GOLDEN_LARGE, "w") as fh:
            json.dump(rec, fh, indent=1, sort_keys=True)
            fh.write("\n")
        print("wrote %s: %s" % (GOLDEN_LARGE, rec))
    if os.path.exists(GOLDEN):
        sys.exit("%s exists: not overwritten" % GOLDEN)
    cases = {}
    for name in MESHES:
        for part, (v, f) in enumerate(decimation_meshes(name)):
            for keep in (True, False):
                for max_rounds in MAX_ROUNDS:
                    cases[case_key(name, part, keep, max_rounds)] = run_case(dev, v, f, keep, max_rounds)
    ws = workspace_cases(dev)
    assert ws["lattice[0] workspace=0xAB"] == ws["lattice[0] workspace=zeros"] \
        == cases[case_key("lattice", 0, True, 200)], "the rounds depend on what the workspace held"
    again = run_case(dev, *decimation_meshes("sphere")[0], True, 200)
    assert again == cases[case_key("sphere", 0, True, 200)], "two runs differ"
    with open(GOLDEN, "w") as fh:
        json.dump({"cases": cases, "workspace": ws}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote %s: %d cases" % (GOLDEN, len(cases)))


if __name__ == "__main__":
    main()
