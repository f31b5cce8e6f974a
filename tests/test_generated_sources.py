"""The generators' text is what tests/golden/generated_sources.json records (tools/source_digests.py, its side layer): every
kernel family, the side products among them, variant and tuning switch of a fixed list of pedigrees, by the SHA-256 of the
source.  Code objects are cached by the hash of their source and the shipped table of measured picks is keyed by it, so a
change of the generators that is not meant to change a kernel must leave every digest as it is.  No GPU; the manifest is
never rewritten from here."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import source_digests as D  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "generated_sources.json")) as f:
    GOLDEN = json.load(f)


def test_the_manifest_covers_the_tools_matrix():
    """Every pedigree is there, and every switch's case differs from the same case without the switch: the family reads it."""
    assert {k.split(" ")[0] for k in GOLDEN} == set(D.SIDE_PEDIGREES)
    for key, value, where, cases in D.SWITCHES + D.SIDE_SWITCHES:
        for case in cases:
            plain = "%s %s" % (where, case)
            assert GOLDEN["%s %s=%s" % (plain, key, value)] != GOLDEN[plain], (key, case)


@pytest.mark.parametrize("name", D.SIDE_PEDIGREES)
def test_every_generated_source_is_the_recorded_one(name, tmp_path, monkeypatch):
    """On a mismatch: the cases, and where today's text of the first lies.  The manifest holds digests, not texts: the differing
    line is shown by `tools/source_digests.py OUT.json --dump DIR` run on both commits and `diff -r` of the two directories."""
    want = {k: v for k, v in GOLDEN.items() if k.split(" ")[0] == name}
    monkeypatch.setattr(D, "TEXTS", {})
    got = D.digests(name, side=True)
    assert sorted(got) == sorted(want), "the set of cases changed: %s" % sorted(set(got) ^ set(want))[:10]
    wrong = [k for k in sorted(want) if got[k] != want[k]]
    if wrong:
        (tmp_path / "first_mismatch.hip").write_bytes(D.TEXTS[got[wrong[0]]])
    assert not wrong, "%d of %d sources differ from the manifest: %s; today's text of the first: %s" % (
        len(wrong), len(want), ", ".join(wrong[:8]), tmp_path / "first_mismatch.hip")
