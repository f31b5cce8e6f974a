"""The text of the kernels added since tests/golden/generated_sources_later.json was written — the characteristic-function
kernel, plain and site-prior, in its four fence levels on the manifest's nineteen pedigrees — is what
tests/golden/generated_sources_newer.json records (tools/source_digests.py --newer).  The two older manifests stay as they are
and their tests go on checking that no existing text has moved; this one pins the new texts the same way.  No GPU; the manifest
is never rewritten from here."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import source_digests as D  # noqa: E402
from famseq_amd.prebuild_sets import SIDE_PRODUCTS_NEWER, SIDE_VARIANTS  # noqa: E402


def manifest(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        return json.load(f)


GOLDEN = manifest("generated_sources_newer.json")
OLDER = dict(manifest("generated_sources.json"), **manifest("generated_sources_later.json"))


def test_the_manifest_covers_the_newer_products():
    assert {k.split(" ")[0] for k in GOLDEN} == set(D.SIDE_PEDIGREES)
    keys = [stem + tail for stem, _, has_prior in SIDE_PRODUCTS_NEWER for tail in [""] + (["_prior"] if has_prior else [])]
    assert keys == ["charfn", "charfn_prior"] and D.NEWER_STEMS == (("charfn", True),)
    assert sorted(GOLDEN) == sorted("%s %s/%d" % (name, key, v) for name in D.SIDE_PEDIGREES for key in keys for v in range(SIDE_VARIANTS))
    assert not set(GOLDEN) & set(OLDER)
    # a new kernel, not another name for an old text; the site-prior form differs from the plain one
    assert not set(GOLDEN.values()) & set(OLDER.values())
    assert all(GOLDEN["%s charfn/%d" % (n, v)] != GOLDEN["%s charfn_prior/%d" % (n, v)] for n in D.SIDE_PEDIGREES for v in range(SIDE_VARIANTS))


@pytest.mark.parametrize("name", D.SIDE_PEDIGREES)
def test_every_newer_source_is_the_recorded_one(name, tmp_path, monkeypatch):
    want = {k: v for k, v in GOLDEN.items() if k.split(" ")[0] == name}
    monkeypatch.setattr(D, "TEXTS", {})
    got = D.later_digests(name, D.NEWER_STEMS)
    assert sorted(got) == sorted(want), "the set of cases changed: %s" % sorted(set(got) ^ set(want))[:10]
    wrong = [k for k in sorted(want) if got[k] != want[k]]
    if wrong:
        (tmp_path / "first_mismatch.hip").write_bytes(D.TEXTS[got[wrong[0]]])
    assert not wrong, "%d of %d sources differ from the manifest: %s; today's text of the first: %s" % (
        len(wrong), len(want), ", ".join(wrong[:8]), tmp_path / "first_mismatch.hip")
