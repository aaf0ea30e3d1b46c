"""The volume ops on an MI355X give the bits they gave before they were moved onto csrc/volume_common.h: every digest of
tests/volume_bits_cases.py equals the `gfx950` section of tests/golden/volume_bits.json (written on an MI355X from a build of the parent
commit)."""
import pytest

import volume_bits_cases as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", B.GROUPS)
def test_volume_bits(hip_backend, group):
    B.check(hip_backend, "gfx950", group)


def test_every_pinned_case_is_still_produced(hip_backend):
    B.check_complete(hip_backend, "gfx950")
