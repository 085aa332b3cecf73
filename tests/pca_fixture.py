"""The PCA fixture (tests/golden/golden_pca.*, tests/golden/pca_*.json) as the tests use it: the models, the rows of every projection case and the
observations of every covariance case, composed once per process and handed out read-only."""
import functools
import os

import numpy as np

import pca_cases as pc
import pca_model as pm
from fixtures import GOLDEN_DIR, load_golden


def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def golden():
    return load_golden("golden_pca")


def model_path(name):
    return os.path.join(GOLDEN_DIR, name + ".json")


@functools.lru_cache(maxsize=None)
def model_text(name):
    """the text of a model file: the kept ones from tests/golden, the composed ones made here and held against the fixture's digest"""
    meta, _ = golden()
    for rec in meta["composed"]:
        if rec["id"] == name:
            text = pc.compose_text(rec["dim"], rec["components"], rec["seed"])
            assert pc.sha256(text.encode()) == rec["sha256"], name
            return text
    return open(model_path(name)).read()


@functools.lru_cache(maxsize=None)
def model(name):
    """(mean, vectors, values) by tests/pca_model.py's parser, which the generator held against CompVMathPCA::read on every bit"""
    mean, vectors, values = pm.parse_text(model_text(name))
    meta, _ = golden()
    for rec in meta["composed"]:
        if rec["id"] == name:
            assert pc.sha256(np.concatenate([mean, vectors.ravel(), values])) == rec["arrays_sha256"], name
    return frozen(mean), frozen(vectors), frozen(values)


def kept_models():
    meta, _ = golden()
    return [r["id"] for r in meta["trained"] + meta["hand"]]


def project_cases():
    return golden()[0]["project"]


@functools.lru_cache(maxsize=None)
def case_rows(cid):
    rec = next(r for r in project_cases() if r["id"] == cid)
    return frozen(pc.reference_rows(rec["n"], rec["dim"]) if rec["rows"] == "reference" else pc.rows(rec["n"], rec["dim"], rec["rows"]))


def expected(cid):
    return golden()[1]["out_" + cid]


@functools.lru_cache(maxsize=None)
def expected_raw(cid):
    """the outputs without a mean: the model's, held against the digest of CompVMath::mulABt's in the fixture"""
    rec = next(r for r in project_cases() if r["id"] == cid)
    out = pm.project(case_rows(cid), None, model(rec["model"])[1])
    assert pc.sha256(out) == rec["raw_sha256"], cid
    return frozen(out)


@functools.lru_cache(maxsize=None)
def covariance_case(n, D):
    """(observations, mean, covariance): the mean is the reference's, the covariance the model's held against the fixture's digest"""
    meta, arrays = golden()
    rec = next(r for r in meta["covariance"] if (r["n"], r["dim"]) == (n, D))
    obs = pc.observations(n, D, rec["seed"])
    mean, cov = pm.covariance(obs)
    assert pm.bits(mean).tobytes() == pm.bits(arrays["mean_%d_%d" % (n, D)]).tobytes() and pc.sha256(cov) == rec["covar_sha256"], (n, D)
    return frozen(obs), frozen(mean), frozen(cov)
