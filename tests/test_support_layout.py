"""The layout of tests/ and tools/: shared code lives in support modules, never in a test module, and a support module can be imported without torch,
without libcompv_hip.so and without a device (tests/test_stream_cases.py and CPU-only collection rely on that).  Standard library only."""
import ast
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUPPORT = ("gpu_support", "fixtures", "host_programs", "stream_order_rig", "gauss_cases", "components_rig", "sht_fit_rig", "sht_segments_rig", "morph_rig",
           "match_rig", "homography_rig", "fast_rig", "hog_rig", "orb_rig", "orb_pyramid_rig", "curvefit_rig", "svm_rig", "undistort_rig", "fresh_memory_cases")


def imported_modules(nodes):
    for n in nodes:
        if isinstance(n, ast.Import):
            yield from ((n.lineno, a.name) for a in n.names)
        elif isinstance(n, ast.ImportFrom):
            yield n.lineno, n.module or ""


def parse(path):
    with open(path) as f:
        return ast.parse(f.read(), path)


def test_no_module_imports_a_test_module():
    """anywhere in a file: several of the imports this rule replaced sat inside functions"""
    found, files = [], 0
    for top in ("tests", "tools"):
        for folder, _, names in os.walk(os.path.join(ROOT, top)):
            for name in sorted(n for n in names if n.endswith(".py")):
                path = os.path.join(folder, name)
                files += 1
                found += ["%s:%d imports %s" % (os.path.relpath(path, ROOT), line, mod) for line, mod in imported_modules(ast.walk(parse(path)))
                          if any(part.startswith("test_") for part in mod.split("."))]
    assert files > 100 and not found, "\n".join(found)


def test_support_modules_import_neither_torch_nor_the_library_at_module_level():
    """module level: the statements an import of the module runs, those inside if / try / with blocks and class bodies included, function bodies not"""
    def top_level(nodes):
        for n in nodes:
            yield n
            if not isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.Lambda)):
                yield from top_level(ast.iter_child_nodes(n))

    found = []
    for name in SUPPORT:
        path = os.path.join(ROOT, "tests", name + ".py")
        found += ["tests/%s.py:%d imports %s" % (name, line, mod) for line, mod in imported_modules(top_level(parse(path).body))
                  if mod.split(".")[0] in ("torch", "compv_amd")]
    assert not found, "\n".join(found)
