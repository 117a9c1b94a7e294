"""Record what the serial decimation queue returns, as digests, for tests/test_decimate_serial_golden.py:
run with the library the later builds are to be compared with (no GPU needed), from the repository
root:

    python tests/golden/make_decimate_serial_parent.py

Writes tests/golden/decimate_serial_parent.json and refuses to overwrite it: the record is of one
library, taken once, before the code it pins is changed.  The cases (see the test's docstring for
why open meshes at boundary_weight 1 are not among the unseeded ones) are listed in the record."""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
from tests.test_decimate_serial_golden import GOLDEN, all_cases, case_key, run_case  # noqa: E402


def main():
    if os.path.exists(GOLDEN):
        sys.exit("%s exists: not overwritten" % GOLDEN)
    cases = {case_key(*c): run_case(*c) for c in all_cases()}
    for c in all_cases():
        assert run_case(*c) == cases[case_key(*c)], "two runs differ: " + case_key(*c)
    with open(GOLDEN, "w") as fh:
        json.dump({"case_list": [case_key(*c) for c in all_cases()], "cases": cases}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote %s: %d cases" % (GOLDEN, len(cases)))


if __name__ == "__main__":
    main()
