"""CPU suite: docs/ENVIRONMENT.md lists every CL_* environment switch the library reads (scripts/env_switches.py regenerates it)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_environment_table_is_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "env_switches.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout


def test_namespace_scope_constants_are_read_once(tmp_path, monkeypatch):
    """`const T g = [] { ... getenv ... }();` at namespace scope runs when the library is loaded, so the table must say `once` for it; the same lambda indented, inside a
    function and without `static`, runs at every call.  (The sources have no namespace-scope constant of this kind at present, so the rule is shown a file of its own.)
    The routing hooks that plan creation reads through read_pack_switches are `call`, which is what lets tests/test_gpu_general_kernels.py switch them in one process."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import env_switches
    finally:
        sys.path.pop(0)
    found = env_switches.collect()
    for name in ("CL_FORCE_GENERAL", "CL_NO_SYS", "CL_NO_STRIP", "CL_NO_RING", "CL_NO_LANE"):
        assert not found[name]["once"], name
    src = tmp_path / "switches.cpp"
    src.write_text('namespace {\n'
                   'const bool g = [] { const char* e = getenv("CL_X"); return e && *e == \'1\'; }();\n'
                   '}\n'
                   'int f() {\n'
                   '    const bool per_call = [] { const char* e = getenv("CL_Y"); return e && *e == \'1\'; }();\n'
                   '    return per_call;\n'
                   '}\n', encoding="utf-8")
    monkeypatch.setattr(env_switches, "SRC", [str(src)])
    found = env_switches.collect()
    assert sorted(found) == ["CL_X", "CL_Y"]
    assert found["CL_X"]["once"]
    assert not found["CL_Y"]["once"]
