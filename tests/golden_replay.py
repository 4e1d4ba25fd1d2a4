"""Recorded outputs of the reference's compiled cores (oracle/_ref), so that
tests comparing against them run where the reference's sources are absent.

By default a test's reference call is answered from tests/golden/<name>.json:
the entry is keyed by test name and call index, and carries a digest of the
call's inputs, so a test whose inputs drift from the recording fails instead
of comparing against stale data.

Re-recording (dev container, oracle/_ref built): run the tests with
MGX_RECORD_GOLDEN=<dir>; every reference call then goes to the live library
and <dir>/<name>.json is rewritten, to be copied over tests/golden/<name>.json.
"""
import hashlib
import json
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _plain(x):
    """ndarrays / numpy scalars / tuples -> JSON-able lists and numbers."""
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in sorted(x.items())}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, np.generic):
        return x.item()
    return x


class GoldenReplay:
    def __init__(self, name):
        self.name = name
        self.record_dir = os.environ.get("MGX_RECORD_GOLDEN")
        self.calls = {}
        if self.record_dir:
            self.data = {}
        else:
            with open(os.path.join(GOLDEN_DIR, name + ".json")) as f:
                self.data = json.load(f)

    @property
    def recording(self):
        return bool(self.record_dir)

    def _key(self):
        # "tests/test_x.py::test_name[param] (call)" -> "test_name[param]"
        test = os.environ["PYTEST_CURRENT_TEST"].split("::", 1)[1].rsplit(" ", 1)[0]
        n = self.calls.get(test, 0)
        self.calls[test] = n + 1
        return f"{test}#{n}"

    def call(self, inputs, live_fn):
        """Returns what live_fn() returned when the entry was recorded (numpy
        arrays come back as nested lists). live_fn runs only when recording."""
        key = self._key()
        digest = hashlib.sha256(
            json.dumps(_plain(inputs), sort_keys=True).encode()).hexdigest()
        if self.recording:
            out = _plain(live_fn())
            self.data[key] = {"inputs_sha256": digest, "out": out}
            os.makedirs(self.record_dir, exist_ok=True)
            with open(os.path.join(self.record_dir, self.name + ".json"), "w") as f:
                json.dump(self.data, f, sort_keys=True, separators=(",", ":"))
                f.write("\n")
            return out
        assert key in self.data, f"no recorded reference output for {key} in {self.name}.json"
        entry = self.data[key]
        assert entry["inputs_sha256"] == digest, \
            f"{key}: inputs differ from the recording in {self.name}.json; re-record"
        return entry["out"]
