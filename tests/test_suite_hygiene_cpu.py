"""The test suite audits itself.  Round 4 spliced 255 lines of tests/test_fullsize_gpu.py in twice; Python keeps the LAST definition of a name, so the lenient round-3 body
of one test shadowed its strict successor for two rounds while the file still collected and passed.  A repeated top-level name in a test module -- or a
repeated method name in a test class -- is an error here, on the CPU, in every round's first check."""
import ast
import os

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _python_files(top):
    for d, _dirs, files in os.walk(top):
        if "__pycache__" in d:
            continue
        for f in sorted(files):
            if f.endswith(".py"):
                yield os.path.join(d, f)


def _repeated_names(body):
    """names bound more than once by def / class statements directly in this body (an `if` / `try` at module level is walked too: a conditional redefinition shadows just the same)"""
    seen, dup = {}, []
    def walk(stmts):
        for n in stmts:
            if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                if n.name in seen:
                    dup.append((n.name, seen[n.name], n.lineno))
                seen[n.name] = n.lineno
            elif isinstance(n, (ast.If, ast.Try, ast.With)):
                for fld in ("body", "orelse", "finalbody"):
                    walk(getattr(n, fld, []) or [])
                for h in getattr(n, "handlers", []) or []:
                    walk(h.body)
    walk(body)
    return dup


def _audit(path):
    tree = ast.parse(open(path).read(), filename=path)
    bad = [("%s:%d" % (os.path.relpath(path, ROOT), l2), "`%s` already defined at line %d" % (name, l1)) for name, l1, l2 in _repeated_names(tree.body)]
    for n in ast.walk(tree):
        if isinstance(n, ast.ClassDef):
            bad += [("%s:%d" % (os.path.relpath(path, ROOT), l2), "`%s.%s` already defined at line %d" % (n.name, name, l1)) for name, l1, l2 in _repeated_names(n.body)]
    return bad


def test_no_test_module_defines_a_name_twice():
    bad = []
    for path in _python_files(HERE):
        bad += _audit(path)
    assert not bad, "shadowed definitions (the later one is the only one pytest runs):\n" + "\n".join("  %s  %s" % b for b in bad)


def test_the_audit_sees_a_shadowed_test(tmp_path):
    # the round-4 accident in miniature: a strict test followed by its lenient twin
    p = tmp_path / "test_x.py"
    p.write_text("def test_a():\n    assert 1 == 2\n\n\ndef helper():\n    pass\n\n\ndef test_a():\n    pass\n\n\nclass TestK:\n    def test_m(self):\n        pass\n    def test_m(self):\n        pass\n")
    found = _audit(str(p))
    assert len(found) == 2 and "`test_a` already defined at line 1" in found[0][1] and "`TestK.test_m`" in found[1][1]
    q = tmp_path / "test_y.py"
    q.write_text("def test_a():\n    pass\n\n\ndef test_b():\n    def inner():\n        pass\n    def inner2():\n        pass\n")
    assert _audit(str(q)) == []


def _test_module_imports(path):
    """the imports of a `tests.test_*` module in this file: `import tests.test_x`, `from tests.test_x import y`, `from tests import test_x`"""
    found = []
    for n in ast.walk(ast.parse(open(path).read(), filename=path)):
        if isinstance(n, ast.Import):
            names = [a.name for a in n.names]
        elif isinstance(n, ast.ImportFrom) and n.level == 0:
            names = ["tests." + a.name for a in n.names] if n.module == "tests" else [n.module or ""]
        else:
            continue
        found += [("%s:%d" % (os.path.relpath(path, ROOT), n.lineno), name) for name in names if name.startswith("tests.test_")]
    return found


def test_no_module_imports_a_test_module(tmp_path):
    # a restatement that a second module needs lives under oracle/, once; a test module is nobody's library
    bad = []
    for top in ("tests", "oracle", "tools"):            # tests/golden/ is walked with tests/
        for path in _python_files(os.path.join(ROOT, top)):
            if os.path.basename(path) not in ("fakes.py", "conftest.py"):
                bad += _test_module_imports(path)
    assert not bad, "a test module imported as a library:\n" + "\n".join("  %s  %s" % b for b in bad)
    p = tmp_path / "m.py"
    p.write_text("from tests import fakes, test_a_cpu as A\nimport tests.test_b_gpu\n\n\ndef f():\n    from tests.test_c_cpu import g\n    from oracle import pixel_ref\n")
    assert [name for _, name in _test_module_imports(str(p))] == ["tests.test_a_cpu", "tests.test_b_gpu", "tests.test_c_cpu"]


def test_the_top_level_of_tests_holds_test_modules_only():
    # a restatement, a bound or a test input that a test needs is a library: it lives under oracle/, not beside the test modules
    bad = sorted(f for f in os.listdir(HERE) if os.path.isfile(os.path.join(HERE, f)) and not (f in ("conftest.py", "fakes.py", "__init__.py") or (f.startswith("test_") and f.endswith(".py"))))
    assert not bad, "tests/ holds only test_*.py, conftest.py, fakes.py and __init__.py at its top level: %s" % bad


def test_product_and_tool_modules_define_no_name_twice():
    # the same accident in the product package, the oracle, bench.py or a probe script would be as silent
    bad = []
    for top in ("unitex_amd", "oracle", "tools"):
        for path in _python_files(os.path.join(ROOT, top)):
            bad += _audit(path)
    for f in ("bench.py", "__graft_entry__.py"):
        bad += _audit(os.path.join(ROOT, f))
    assert not bad, "\n".join("  %s  %s" % b for b in bad)
