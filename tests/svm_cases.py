"""The SVM cases the fixture generator (tests/golden/make_golden_svm.py) and the tests share: which models exist, how the trained ones' training sets and
every model's queries are drawn (seeded, numpy's legacy generator: stable from version to version), and the hand-composed model files that reach
what training will not give (composed again by every process that needs them: only the trained files are kept under tests/golden/).  Shapes follow the kernels: svm_kvalues_kernel stages 32 columns at a time and sums whole groups of 16, a workgroup owns
64 queries x 64 support vectors; the coefficient dot groups by 16 from a segment's start."""
import atexit
import hashlib
import json
import os
import shutil
import tempfile

import numpy as np

import svm_model as sm

# id: kernel, D, classes, gamma, query type, queries.  A gamma of 1 / D is written by %g with six digits: the file's value is not the trained one.
TRAINED = [
    dict(id="rbf_d1_c2", kernel=sm.RBF, D=1, classes=2, gamma=0.5, qtype="f32", nq=24),
    dict(id="rbf_d2_c2", kernel=sm.RBF, D=2, classes=2, gamma=1.0 / 3, qtype="f64", nq=24),
    dict(id="rbf_d15_c2", kernel=sm.RBF, D=15, classes=2, gamma=1.0 / 15, qtype="f32", nq=24),
    dict(id="rbf_d16_c5", kernel=sm.RBF, D=16, classes=5, gamma=1.0 / 16, qtype="f32", nq=24),
    dict(id="rbf_d17_c2", kernel=sm.RBF, D=17, classes=2, gamma=1.0 / 17, qtype="f64", nq=24),
    dict(id="rbf_d19_c3", kernel=sm.RBF, D=19, classes=3, gamma=1.0 / 19, qtype="f32", nq=24),
    dict(id="rbf_d31_c2", kernel=sm.RBF, D=31, classes=2, gamma=1.0 / 31, qtype="f32", nq=24),
    dict(id="rbf_d32_c3", kernel=sm.RBF, D=32, classes=3, gamma=1.0 / 32, qtype="f64", nq=24),
    dict(id="rbf_d33_c2", kernel=sm.RBF, D=33, classes=2, gamma=1.0 / 33, qtype="f32", nq=257),
    dict(id="rbf_d36_c2", kernel=sm.RBF, D=36, classes=2, gamma=1.0 / 36, qtype="f64", nq=24, sv_queries=4),
    dict(id="lin_d21_c3", kernel=sm.LINEAR, D=21, classes=3, gamma=0.0, qtype="f64", nq=257),
]
PER_CLASS = 6          # training vectors of a class
N_SIZES = (1, 63, 64, 65, 257)          # query counts around the workgroup's 64, taken as prefixes of a 257-query case


def _seed(cid):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(cid)) % (1 << 31)


def training_set(c):
    """-> (float64 vectors holding float32 values (classes * PER_CLASS, D), int32 labels): one cluster per class"""
    rng = np.random.RandomState(_seed(c["id"]))
    centres = rng.uniform(0.0, 1.0, (c["classes"], c["D"]))
    x = np.concatenate([centres[k] + 0.25 * rng.standard_normal((PER_CLASS, c["D"])) for k in range(c["classes"])])
    y = np.repeat(np.arange(c["classes"]) * 3 - 2, PER_CLASS).astype(np.int32)          # labels -2, 1, 4, ...
    return x.astype(np.float32).astype(np.float64), y


def _text(values, digits):
    return [[("%." + str(digits) + "g") % v for v in row] for row in values]


def hand_models():
    """-> [dict(id, kernel, gamma_text, sv_text, coef_text, rho_text, n_sv, label, D, qtype, nq, ...)]: every number is the TEXT that goes into the file"""
    out = []
    rng = np.random.RandomState(77)

    def compose(cid, kernel, D, n_sv, label, gamma_text, qtype, nq, coef=None, rho=None, sv=None, **more):
        nc, l = len(n_sv), int(sum(n_sv))
        sv_text = sv if sv is not None else _text(rng.uniform(-1.0, 1.0, (l, D)), 8)
        coef_text = coef if coef is not None else _text(rng.uniform(-2.0, 2.0, (nc - 1, l)), 16)
        rho_text = rho if rho is not None else ["%g" % v for v in rng.uniform(-0.5, 0.5, nc * (nc - 1) // 2)]
        out.append(dict(id=cid, kernel=kernel, D=D, gamma_text=gamma_text, sv_text=sv_text, coef_text=coef_text, rho_text=rho_text, n_sv=list(n_sv), label=list(label),
                        qtype=qtype, nq=nq, classes=nc, **more))

    # segment lengths 1, 17, 32 and 16, 16: the coefficient dot's groups start at a segment's start, not at 0; labels negative and out of order
    compose("hand_nsv_1_17_32", sm.RBF, 19, [1, 17, 32], [7, -3, 0], "0.0526316", "f32", 24)
    compose("hand_nsv_16_16", sm.RBF, 17, [16, 16], [5, -5], "0.05", "f64", 24)
    compose("hand_lin_nsv_33_2_15", sm.LINEAR, 36, [33, 2, 15], [-1, -2, 3], None, "f32", 24)
    # two staging chunks + 3 columns, RBF and LINEAR; five classes and one column on the LINEAR path
    compose("hand_d67_c3", sm.RBF, 67, [5, 9, 6], [2, 0, 1], "0.0149254", "f32", 24)
    compose("hand_lin_d67_c2", sm.LINEAR, 67, [7, 6], [1, -1], None, "f64", 24)
    compose("hand_lin_d16_c5", sm.LINEAR, 16, [3, 4, 2, 5, 3], [4, 3, 2, 1, 0], None, "f32", 24)
    compose("hand_lin_d1_c2", sm.LINEAR, 1, [2, 3], [-7, 7], None, "f64", 24)
    # more than one workgroup of support vectors (64 per workgroup), an odd count
    compose("hand_l67", sm.RBF, 5, [40, 27], [1, -1], "0.3", "f32", 65)
    # the HOG default of a 64 x 128 crop: 118 staging chunks and a tail of 4 columns; short SV texts keep the file small
    compose("hand_d3780", sm.RBF, 3780, [1, 2], [1, -1], "0.001", "f32", 8, sv=[[str(v) for v in row] for row in rng.randint(0, 2, (3, 3780))],
            coef=[["0.75", "-1.5", "0.5"]], rho=["0.0625"], spread=(0.0, 1.0))
    # gamma * distance around and beyond 708.4: the lower clip of exp_ref; the product with the table's scale may be subnormal
    compose("hand_clip", sm.RBF, 2, [2, 2], [1, 2], "1", "f64", 24, sv=[["0", "0"], ["0.5", "0"], ["0", "0.25"], ["-0.5", "-0.5"]], spread=(18.0, 19.5))
    compose("hand_clip_far", sm.RBF, 2, [1, 1], [1, 2], "1000", "f32", 8, sv=[["0", "0"], ["1", "1"]], spread=(5.0, 40.0))
    # decisions exactly 0: zero coefficients, rho 0 -- every pair votes for its second class
    compose("hand_zero", sm.RBF, 4, [2, 2, 2], [10, 20, 30], "0.5", "f32", 8, coef=[["0"] * 6, ["0"] * 6], rho=["0", "0", "0"])
    # a three-way tie: dec = (1, -1, 1) -> one vote each -> label[0]
    compose("hand_tie", sm.LINEAR, 4, [2, 2, 2], [30, 10, 20], None, "f64", 8, coef=[["0"] * 6, ["0"] * 6], rho=["-1", "1", "-1"])
    return out


def write_hand_model(path, h):
    sm.write_model_file(path, h["kernel"], h["gamma_text"], h["sv_text"], h["coef_text"], h["rho_text"], h["n_sv"], h["label"])


def all_cases():
    return TRAINED + hand_models()


def queries(c, model):
    """The case's queries, (nq, D) float32 or float64; sv_queries: the first ones EQUAL support vectors of the parsed model (K = 1 exactly)"""
    rng = np.random.RandomState(_seed(c["id"]) ^ 0x5eed)
    lo, hi = c.get("spread", (-0.5, 1.5))
    x = rng.uniform(lo, hi, (c["nq"], c["D"]))
    if "spread" not in c:
        near = rng.randint(0, model.l, c["nq"] // 2)          # half of them near support vectors, so that K is not tiny everywhere
        x[:len(near)] = model.sv[near] + 0.1 * rng.standard_normal((len(near), c["D"]))
    x = x.astype(np.float32) if c["qtype"] == "f32" else x
    for i in range(c.get("sv_queries", 0)):
        x[i] = model.sv[(i * 5) % model.l]
    return np.ascontiguousarray(x)


def exp_inputs():
    """a few thousand inputs across [-750, 10] with both clip bounds, their neighbours and 0"""
    rng = np.random.RandomState(11)
    special = [0.0, -0.0, sm.EXP_MIN, sm.EXP_MAX, np.nextafter(sm.EXP_MIN, 0.0), np.nextafter(sm.EXP_MIN, -1e3), np.nextafter(sm.EXP_MAX, 0.0), -750.0, 10.0, -1.0, 1.0,
               -708.0, -709.0, -745.2, 1e-300, -1e-300, 5e-324]
    return np.concatenate([np.array(special), np.linspace(-750.0, 10.0, 800), rng.uniform(-750.0, 10.0, 800), -np.exp(rng.uniform(-30.0, 6.5, 400))])


_hand_dir = None


def model_path(cid):
    """A trained model's file lies under tests/golden/ (the reference wrote it).  A hand-composed one is a function of hand_models() alone: it is written
    on first use into a temporary directory of this process (the fixture records its SHA-256), not kept in the repository."""
    global _hand_dir
    if not cid.startswith("hand_"):
        return os.path.join(sm.GOLDEN, "svm_%s.model" % cid)
    if _hand_dir is None:
        _hand_dir = tempfile.mkdtemp(prefix="svm_hand_")
        atexit.register(shutil.rmtree, _hand_dir, True)
    path = os.path.join(_hand_dir, "svm_%s.model" % cid)
    if not os.path.exists(path):
        write_hand_model(path, next(h for h in hand_models() if h["id"] == cid))
    return path


def file_sha256(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


_golden = None


def golden():
    """-> (meta of golden_svm.json, arrays of golden_svm.npz), loaded once and shared"""
    global _golden
    if _golden is None:
        with open(os.path.join(sm.GOLDEN, "golden_svm.json")) as f:
            meta = json.load(f)
        _golden = (meta, dict(np.load(os.path.join(sm.GOLDEN, "golden_svm.npz"))))
    return _golden


def recorded_model(c):
    """The model of a case as the generator saw it: a trained file's arrays as recorded in the fixture (tests/svm_model.py's parse of the file, which gave
    the reference's own K, dec and labels); a hand-composed file, whose text must have the recorded SHA-256, parsed again."""
    meta, A = golden()
    rec = next(r for r in meta["cases"] if r["id"] == c["id"])
    cid = c["id"]
    if not rec["trained"]:
        assert file_sha256(model_path(cid)) == rec["sha256"], "%s: the composed file is not the one the fixture was made from" % cid
        return sm.parse(model_path(cid))
    return sm.Model(rec["kernel"], float.fromhex(rec["gamma"]), A["sv_" + cid], A["coef_" + cid], A["rho_" + cid], A["nsv_" + cid], A["label_" + cid])


def padded(x, stride, sentinel):
    """the queries staged at `stride` elements a row, the padding filled with a sentinel that no call may read into a result"""
    out = np.full((len(x), stride), sentinel, x.dtype)
    out[:, :x.shape[1]] = x
    return out


BAD_FILES = {          # item F's refusals on hand-made files: name -> (what to do with a good two-class RBF file's text)
    "sparse_gap": lambda t: t.replace(" 2:", " 3:", 1),
    "sparse_short": lambda t: t.rstrip("\n").rsplit(" ", 2)[0] + " \n",
    "poly": lambda t: t.replace("kernel_type rbf", "kernel_type polynomial\ndegree 3"),
    "sigmoid": lambda t: t.replace("kernel_type rbf", "kernel_type sigmoid"),
    "precomputed": lambda t: t.replace("kernel_type rbf", "kernel_type precomputed"),
    "one_class": lambda t: t.replace("svm_type c_svc", "svm_type one_class"),
    "nu_svc": lambda t: t.replace("svm_type c_svc", "svm_type nu_svc"),
    "epsilon_svr": lambda t: t.replace("svm_type c_svc", "svm_type epsilon_svr"),
    "nu_svr": lambda t: t.replace("svm_type c_svc", "svm_type nu_svr"),
    "truncated_lines": lambda t: "\n".join(t.split("\n")[:-3]) + "\n",
    "truncated_header": lambda t: t[:t.index("nr_sv")],
    "truncated_mid_line": lambda t: t[:len(t) - 25],
    "garbage_number": lambda t: t.replace("gamma ", "gamma x", 1),
    "unknown_word": lambda t: t.replace("nr_class", "classes", 1),
    "nr_sv_sum": lambda t: t.replace("total_sv ", "total_sv 1", 1),
    "empty": lambda t: "",
}


def write_bad_file(path, name):
    with open(model_path("rbf_d17_c2")) as f:
        good = f.read()
    bad = BAD_FILES[name](good)
    assert bad != good, name
    with open(path, "w") as f:
        f.write(bad)
