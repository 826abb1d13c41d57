"""The package's import layers: the host runtime (sam6d_hip.runtime) sits under every module, the PEM matching pipeline
(sam6d_hip.pem) under none of them.  Each module is imported in a fresh interpreter, with SAM6D_LIB pointing at a file that does not
exist: an import that loaded the shared library would fail there."""
import os
import subprocess
import sys

import pytest

from tests._util import PKG

MODULES = ("runtime", "ops", "encoder", "vit", "dinov2", "ism", "inputs", "amg", "samfront", "samenc", "samdec")

CHILD = ("import sys; sys.path.insert(0, %r)\n"
         "import sam6d_hip.%s\n"
         "print(' '.join(sorted(m for m in sys.modules if m == 'sam6d_hip' or m.startswith('sam6d_hip.'))))\n")


@pytest.mark.parametrize("name", MODULES)
def test_module_imports_without_the_pipeline(name, tmp_path):
    env = dict(os.environ, SAM6D_LIB=str(tmp_path / "no_such_library.so"))
    r = subprocess.run([sys.executable, "-c", CHILD % (PKG, name)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    loaded = set(r.stdout.split())
    assert "sam6d_hip." + name in loaded
    assert "sam6d_hip.pem" not in loaded, sorted(loaded)
    if name == "runtime":
        assert loaded == {"sam6d_hip", "sam6d_hip._lib", "sam6d_hip.runtime"}, sorted(loaded)
