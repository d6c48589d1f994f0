"""The pairing tail on one wave of the device interpreter (dp_vm_run of
tests/device/fp_probe.hip), on the crafted inputs of tests/pairing_cases.py: the tower and
pairing ops of tools/fpvm/alg.py as one-op programs at W = 64 and W = 16 on every case, and the
product's fold / final / final1 / gfin / qcmil / gmil / rs programs on one case per class
(tests/test_vm_host_pairing.py runs them on every case on the host). Device == slot-level
simulator, and the simulator == the plain-integer reference (tests/pairing_vm.py)."""
import ctypes
import os

import pytest

import pairing_cases as pcs
import pairing_vm
from test_vm_host_pairing import NRUNS
from vm_helpers import ROOT

pytestmark = pytest.mark.gpu

PROBE = os.path.join(ROOT, "tests", "device", "_build", "libfpprobe.so")


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        pytest.fail("%s is missing: run build() (make -C consensus_overlord_amd) first" % PROBE)
    return ctypes.CDLL(PROBE)


@pytest.mark.parametrize("W", pairing_vm.WIDTHS)
@pytest.mark.parametrize("name", pairing_vm.OPS)
def test_op_program_on_every_case_on_device(probe, name, W):
    assert pairing_vm.run_op(probe, True, name, W) == NRUNS[name]


@pytest.mark.parametrize("W", pairing_vm.WIDTHS)
def test_eq_one_on_representatives_equal_only_modulo_p_on_device(probe, W):
    assert pairing_vm.run_eq_one_raw(probe, True, W) == 3


@pytest.mark.parametrize("name", pairing_vm.PRODUCT)
def test_product_program_on_one_case_per_class_on_device(probe, name):
    classes = {"final": pcs.FINAL_CLASSES, "fold": pcs.FINAL_CLASSES, "final1": pcs.FE_CLASSES, "gfin": pcs.GFIN_CLASSES,
               "gmil": ("scaled", "golden", "bilinear"), "qcmil": ("scaled", "golden", "bilinear"),
               "rs": pcs.RS_Z + ("random",)}   # every rs value is a class of its own
    assert pairing_vm.run_product(probe, True, name, one_per_class=True) == len(classes[name])
