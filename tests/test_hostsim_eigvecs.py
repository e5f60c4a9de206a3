"""CPU tier: eigvecs(ps, select; shifted, method="backsub") — periodic back-substitution (csrc/psd_evec.h, driver
psd_evec_host.inl) on the TEST-ONLY serial simulation of the device code, against the reference's test problems
(test/vectors.jl), the reordering method and a numpy prototype of the algorithm."""
import pytest

import evec_cases as vc


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("p", [1, 5])
def test_vectors_jl_problems(sim_engine, cplx, p):
    vc.case_vectors_jl(sim_engine, cplx, p)


@pytest.mark.parametrize("cplx", [False, True])
def test_agrees_with_ordschur(sim_engine, cplx):
    vc.case_vs_ordschur(sim_engine, cplx)


@pytest.mark.parametrize("lr", ["L", "R"])
def test_conjugate_pairs(sim_engine, lr):
    vc.case_pairs(sim_engine, lr)


def test_negative_eigenvalue_even_period(sim_engine):
    vc.case_negative_even_p(sim_engine)


@pytest.mark.parametrize("cplx", [False, True])
def test_repeated_eigenvalues(sim_engine, cplx):
    vc.case_repeated(sim_engine, cplx)


@pytest.mark.parametrize("cplx", [False, True])
def test_zero_eigenvalue(sim_engine, cplx):
    vc.case_zero(sim_engine, cplx)


def test_argument_errors(sim_engine):
    vc.case_errors(sim_engine)


@pytest.mark.parametrize("cplx", [False, True])
def test_several_chunks(sim_engine, cplx):
    vc.case_chunks(sim_engine, cplx)


def test_rescaled_columns(sim_engine):
    vc.case_rescale(sim_engine)


@pytest.mark.parametrize("cplx", [False, True])
def test_partial_schur(sim_engine, cplx):
    vc.case_partial(sim_engine, cplx)

