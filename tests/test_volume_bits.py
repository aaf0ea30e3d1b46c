"""The volume ops on the emulator give the bits they gave before they were moved onto csrc/volume_common.h: every digest of
tests/volume_bits_cases.py equals the `emu` section of tests/golden/volume_bits.json (written from the parent commit)."""
import json

import pytest

import volume_bits_cases as B


@pytest.mark.parametrize("group", B.GROUPS)
def test_volume_bits(emu_backend, group):
    B.check(emu_backend, "emu", group)


def test_every_pinned_case_is_still_produced(emu_backend):
    B.check_complete(emu_backend, "emu")


def test_both_sections_pin_the_same_cases():
    doc = json.load(open(B.GOLDEN))
    assert set(doc) == {"emu", "gfx950"} and sorted(doc["emu"]) == sorted(doc["gfx950"]) and len(doc["emu"]) > 0
