"""tests/svm_model.py -- the numpy definition of SVM prediction (include/compv_hip.h, "SVM prediction") -- against the fixture the compiled reference
made (tests/golden/make_golden_svm.py): kernel values, decision values and labels of every stored query byte for byte, exp_ref alone, the parser
against the model files' recorded arrays, and the refusals of item F on hand-made bad files.  No GPU."""
import math

import numpy as np
import pytest

import svm_cases as sc
import svm_model as sm

CASES = sc.all_cases()


def test_the_fixture_lists_every_case_once():
    meta, A = sc.golden()
    assert [r["id"] for r in meta["cases"]] == [c["id"] for c in CASES]
    assert [r["id"] for r in meta["cases"] if r["trained"]] == [c["id"] for c in sc.TRAINED]
    assert all(sc.file_sha256(sc.model_path(r["id"])) == r["sha256"] for r in meta["cases"])          # kept and composed files alike
    assert {c["D"] for c in CASES} >= {1, 2, 15, 16, 17, 19, 31, 32, 33, 36, 3780} and {c["classes"] for c in CASES} >= {2, 3, 5}
    assert {c["kernel"] for c in CASES} == {sm.LINEAR, sm.RBF} and {c["qtype"] for c in CASES} == {"f32", "f64"}
    assert max(c["nq"] for c in CASES) == max(sc.N_SIZES) == 257
    assert meta["exp_inputs"] == len(sc.exp_inputs()) >= 2000


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["id"])
def test_parser_and_model_equal_the_fixture(c):
    _, A = sc.golden()
    cid = c["id"]
    m = sm.parse(sc.model_path(cid))
    rec = sc.recorded_model(c)
    assert (m.kernel, m.nr_class, m.l, m.dim) == (rec.kernel, rec.nr_class, rec.l, rec.dim) == (c["kernel"], c["classes"], A["K_" + cid].shape[1], c["D"])
    assert np.float64(m.gamma).tobytes() == np.float64(rec.gamma).tobytes()
    for got, exp in ((m.sv, rec.sv), (m.sv_coef, rec.sv_coef), (m.rho, rec.rho), (m.n_sv, rec.n_sv), (m.label, rec.label)):
        assert got.dtype == exp.dtype and got.shape == exp.shape and got.tobytes() == exp.tobytes()
    X = sc.queries(c, m)
    assert X.dtype == (np.float32 if c["qtype"] == "f32" else np.float64) and X.shape == (c["nq"], c["D"])
    labels, dec, K = sm.predict(m, X)
    assert K.tobytes() == A["K_" + cid].tobytes() and dec.tobytes() == A["dec_" + cid].tobytes() and labels.tobytes() == A["lab_" + cid].tobytes()


def test_the_edge_cases_are_what_they_claim():
    _, A = sc.golden()
    assert (A["K_rbf_d36_c2"][np.arange(4), (np.arange(4) * 5) % A["K_rbf_d36_c2"].shape[1]] == 1.0).all()          # a query equal to a support vector
    clip = A["K_hand_clip"]
    floor = sm.exp_ref(np.array([sm.EXP_MIN]))[0]
    assert (clip == floor).any() and (clip > floor).any() and (A["K_hand_clip_far"] == floor).all()          # gamma * distance on both sides of 708.4
    assert not A["dec_hand_zero"].any() and (A["lab_hand_zero"] == 30).all()                                  # dec == 0 votes for j
    assert (A["dec_hand_tie"] == [1.0, -1.0, 1.0]).all() and (A["lab_hand_tie"] == 30).all()                  # a three-way tie: label[0]
    assert float.fromhex(next(r for r in sc.golden()[0]["cases"] if r["id"] == "rbf_d19_c3")["gamma"]) == 0.0526316 != 1.0 / 19          # %g shortened it
    assert {len(set(A["lab_" + c["id"]].tolist())) for c in CASES} >= {1, 2, 3, 5}
    odd = sc.recorded_model(next(c for c in CASES if c["id"] == "hand_nsv_1_17_32")).label
    assert sorted(odd.tolist()) != odd.tolist() and odd.min() < 0          # labels out of order, one negative


def test_exp_ref_equals_the_reference():
    _, A = sc.golden()
    x = sc.exp_inputs()
    assert sm.exp_ref(x).tobytes() == A["exp_out"].tobytes()
    assert sm.EXP_MIN in x and sm.EXP_MAX in x and 0.0 in x and x.min() == -750.0
    assert sm.exp_ref(np.array([0.0]))[0] == 1.0
    ok = (x > -700) & (x < 700)          # (at ExpMax itself the reference's scale overflows: it returns infinity, and so does the model)
    assert np.allclose(A["exp_out"][ok], np.exp(x[ok]), rtol=1e-13, atol=0)          # and it is an exponential
    assert all(int(sm.EXP_TABLE[i]) == (np.float64(math.pow(2.0, i / 2048.0)).view(np.uint64) & np.uint64((1 << 52) - 1)) for i in (0, 1, 1024, 2047))


@pytest.mark.parametrize("name", sorted(sc.BAD_FILES))
def test_bad_files_are_refused(tmp_path, name):
    path = str(tmp_path / (name + ".model"))
    sc.write_bad_file(path, name)
    with pytest.raises(sm.ModelFileError):
        sm.parse(path)


def test_a_missing_file_is_refused(tmp_path):
    with pytest.raises(OSError):
        sm.parse(str(tmp_path / "nothing.model"))
