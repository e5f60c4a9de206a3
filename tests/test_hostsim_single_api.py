"""CPU tier: the single-problem entries of the C ABI through raw ctypes (argument codes, return value == *info, slots,
switches, signatures, statistics), on the TEST-ONLY serial simulation (tests/hostsim)."""
import pytest

import single_api_cases as sc

ENTRY_IDS = [("z" if c else "d") + "_" + f for f, c in sc.ENTRIES]
SIZE_IDS = [f"n{n}p{p}" for n, p in sc.SIZES]
REPEATS = [("pschur", False, False), ("pschur", True, False), ("pschur", True, True), ("gpschur", False, True)]


@pytest.mark.parametrize("fam,cplx", sc.ENTRIES, ids=ENTRY_IDS)
def test_arg_codes(sim_engine, fam, cplx):
    sc.case_arg_codes(sim_engine, fam, cplx)


@pytest.mark.parametrize("n,p", sc.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("cplx", [False, True])
def test_pschur(sim_engine, cplx, n, p):
    sc.case_pschur(sim_engine, cplx, n, p)


@pytest.mark.parametrize("cplx,n,p", [(c, n, p) for c in (False, True) for n, p in sc.SIZES if p > 1 or not c])
def test_signed(sim_engine, cplx, n, p):
    sc.case_signed(sim_engine, cplx, n, p)


@pytest.mark.parametrize("n,p", sc.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("fam,cplx", [("pschur_hess", False), ("pschur_hess", True), ("gpschur_hess", False)])
def test_hess(sim_engine, fam, cplx, n, p):
    sc.case_hess(sim_engine, fam, cplx, n, p)


@pytest.mark.parametrize("n,p", sc.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("cplx", [False, True])
def test_phessenberg(sim_engine, cplx, n, p):
    sc.case_phessenberg(sim_engine, cplx, n, p)


@pytest.mark.parametrize("n,p", sc.SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("cplx", [False, True])
def test_rphessenberg(sim_engine, cplx, n, p):
    sc.case_rphessenberg(sim_engine, cplx, n, p)


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("n", sc.ORD_N)
@pytest.mark.parametrize("cplx", [False, True])
def test_ordschur(sim_engine, cplx, n, p):
    sc.case_ordschur(sim_engine, cplx, n, p)


@pytest.mark.parametrize("p", [2, 3])
@pytest.mark.parametrize("n", sc.ORD_N)
@pytest.mark.parametrize("cplx", [False, True])
def test_gordschur(sim_engine, cplx, n, p):
    sc.case_gordschur(sim_engine, cplx, n, p)


@pytest.mark.parametrize("fam,cplx,signed", REPEATS)
def test_repeat_calls(sim_engine, fam, cplx, signed):
    sc.case_repeat_calls(sim_engine, fam, cplx, signed)
