"""CPU tier: geigvecs(P, select; shifted) — eigenvectors of signed and singular periodic products (csrc/psd_gevec.h,
driver psd_gevec_host.inl) on the TEST-ONLY serial simulation of the device code, against the result contract, the
dense signed product, eigvecs(method="backsub") and a numpy prototype."""
import pytest

import gevec_cases as gc


@pytest.mark.parametrize("spat", ["alt", "tfft"])
@pytest.mark.parametrize("lr", ["L", "R"])
@pytest.mark.parametrize("cplx", [False, True])
def test_signed_forms(sim_engine, cplx, lr, spat):
    gc.case_signed(sim_engine, cplx, lr, spat)


@pytest.mark.parametrize("cplx", [False, True])
def test_end_to_end_signed(sim_engine, cplx):
    gc.case_end_to_end(sim_engine, cplx)


@pytest.mark.parametrize("lr", ["L", "R"])
@pytest.mark.parametrize("cplx", [False, True])
def test_zero_and_infinite_eigenvalues(sim_engine, cplx, lr):
    gc.case_zero_infinite(sim_engine, cplx, lr)


@pytest.mark.parametrize("cplx", [False, True])
def test_periodic_schur_zero_eigenvalue(sim_engine, cplx):
    gc.case_plain_zero(sim_engine, cplx)


@pytest.mark.parametrize("lr", ["L", "R"])
def test_conjugate_pairs(sim_engine, lr):
    gc.case_pairs(sim_engine, lr)


@pytest.mark.parametrize("cplx", [False, True])
def test_pair_across_chunks(sim_engine, cplx):
    gc.case_chunk_pair(sim_engine, cplx)


@pytest.mark.parametrize("cplx", [False, True])
def test_repeated_eigenvalues(sim_engine, cplx):
    gc.case_repeated(sim_engine, cplx)


def test_rescaled_columns(sim_engine):
    gc.case_rescale(sim_engine)


@pytest.mark.parametrize("lr", ["L", "R"])
@pytest.mark.parametrize("cplx", [False, True])
def test_all_true_matches_eigvecs(sim_engine, cplx, lr):
    gc.case_vs_eigvecs(sim_engine, cplx, lr)


def test_argument_errors(sim_engine):
    gc.case_errors(sim_engine)
