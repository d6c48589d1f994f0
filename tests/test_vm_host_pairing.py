"""The tower and pairing ops of tools/fpvm/alg.py as one-op programs, and the product's fold /
final / final1 / gfin / qcmil / gmil / rs programs, on the crafted inputs of
tests/pairing_cases.py, through the interpreter's own code (consensus_overlord_amd/csrc/fpvm.hpp
exec, host build) in both interpreter modes (each lane's own blocks, and every wave-uniform block
for every lane): interpreter == slot-level simulator == DAG evaluation == the plain-integer
reference (tests/pairing_vm.py, tests/pairing_ref.py), on every case of every program in both
modes. Simulations are kept per process, so the second mode costs the interpreter runs alone."""
import pytest

import pairing_vm
from test_host_harness import hx  # noqa: F401  (module fixture: builds libhx.so)

NRUNS = {"f12_mul": 7, "f12_sqr": 14, "f12_inv": 14, "f12_frob": 14 + 26, "f12_mul_014": 5, "f12_cyc_sqr": 4, "f12_exp_x": 4,
         "final_exp": 26, "f12_eq_one": 52, "miller_aff": 5, "miller_proj": 5, "miller_two": 2}
PRODUCT_RUNS = {"final": 10, "fold": 10, "final1": 26, "gfin": 3, "qcmil": 5, "gmil": 5, "rs": 5}


def test_every_listed_op_has_a_program():
    assert set(NRUNS) == set(pairing_vm.OPS) and len(pairing_vm.OPS) == 12
    assert {n: len(pairing_vm.op_runs(n)) for n in pairing_vm.OPS} == NRUNS
    assert set(PRODUCT_RUNS) == set(pairing_vm.PRODUCT)
    assert {n: len(pairing_vm.product_runs(n)) for n in pairing_vm.PRODUCT} == PRODUCT_RUNS


@pytest.mark.parametrize("any_all", [0, 1])
@pytest.mark.parametrize("W", pairing_vm.WIDTHS)
@pytest.mark.parametrize("name", pairing_vm.OPS)
def test_op_program_on_every_case(hx, name, W, any_all):  # noqa: F811
    assert pairing_vm.run_op(hx, False, name, W, any_all) == NRUNS[name]


@pytest.mark.parametrize("any_all", [0, 1])
@pytest.mark.parametrize("W", pairing_vm.WIDTHS)
def test_eq_one_on_representatives_equal_only_modulo_p(hx, W, any_all):  # noqa: F811
    assert pairing_vm.run_eq_one_raw(hx, False, W, any_all) == 3


@pytest.mark.parametrize("any_all", [0, 1])
@pytest.mark.parametrize("name", pairing_vm.PRODUCT)
def test_product_program_on_every_case(hx, name, any_all):  # noqa: F811
    assert pairing_vm.run_product(hx, False, name, any_all) == PRODUCT_RUNS[name]
