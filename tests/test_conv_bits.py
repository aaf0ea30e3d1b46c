"""The conv entry points give the bits they gave before their sources were moved onto csrc/conv_internal.h: every digest of
tests/conv_bits_cases.py equals tests/golden/conv_bits.json -- the `emu` section on the CPU emulator, the `gfx950` section (written on an
MI355X from a build of the parent commit) on the HIP library."""
import pytest

import conv_bits_cases as B


@pytest.mark.parametrize("group", B.GROUPS)
def test_conv_bits(emu_backend, group):
    B.check(emu_backend, "emu", group)


def test_every_pinned_case_is_still_produced(emu_backend):
    B.check_complete(emu_backend, "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("group", B.GROUPS)
def test_conv_bits_gpu(hip_backend, group):
    B.check(hip_backend, "gfx950", group)


@pytest.mark.gpu
def test_every_pinned_case_is_still_produced_gpu(hip_backend):
    B.check_complete(hip_backend, "gfx950")
