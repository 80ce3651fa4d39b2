"""The HybridFusion plan pinned on the CPU: over a grid of shapes, modes and plan switches the
library's host-only queries -- mmf_hybrid_saved_bytes, mmf_hybrid_workspace_bytes,
mmf_hybrid_saved_region (every modality, the classifier hidden layer), mmf_hybrid_lean_l1,
mmf_hybrid_train_sync_bytes and, per switch setting, mmf_hybrid_plan_flags -- answer what
tests/golden/hybrid_layout.json recorded (tests/golden/gen_hybrid_layout.py: the grid and the
queries).  Every value is an integer and must be equal: a change of any plan decision that moves a
byte of `saved` or the workspace shows here, without a GPU.

The workspace size depends on the device's CU count (the split counts of the weight gradients):
256 on an MI355X, and 256 as the library's fallback with no device, so the fixture holds on both.
"""
import json

import pytest

import gen_hybrid_layout as gen


@pytest.fixture(scope="module")
def nat(pkg_on_path):
    import mmf_native
    try:
        mmf_native.lib()
    except RuntimeError as e:
        pytest.fail(f"libmmfusion.so not built: {e}")
    return mmf_native


def test_hybrid_layout_matches_fixture(nat):
    fixture = json.loads(gen.FIXTURE.read_text())
    # the fixture was made for this grid
    assert fixture["shapes"] == list(gen.SHAPES)
    assert fixture["modes"] == [list(m) for m in gen.MODES]
    assert fixture["settings"] == [list(s) for s in gen.SETTINGS]
    want = gen.unpack(fixture)
    got = gen.collect(nat)
    assert got["plan_flags"] == want["plan_flags"]
    assert len(got["cases"]) == len(want["cases"]) == len(gen.SHAPES) * len(gen.MODES) * len(gen.SETTINGS)
    names = [(s, m, k) for s in gen.SHAPES for m in gen.MODES for k in gen.SETTINGS]
    wrong = [(name, g, w) for name, g, w in zip(names, got["cases"], want["cases"]) if g != w]
    assert not wrong, f"{len(wrong)} of {len(names)} cases differ; the first: {wrong[0]}"
