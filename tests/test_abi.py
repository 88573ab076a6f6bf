"""CPU suite: the C-ABI library loads and exports every symbol include/mrslam_hip.h declares."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "mrslam_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mrs_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from mr_slam_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(_lib.LIB_PATH)
    names = _declared_symbols()
    assert len(names) >= 10
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.mrs_abi_version() == 1


def test_no_cpu_fallback_without_gpu():
    """Without a GPU the product path must fail loudly (MRS_ERR_NO_DEVICE), never compute."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mr_slam_amd import _lib
    with pytest.raises(_lib.MrsError):
        _lib.ctx(0)
    import numpy as np
    from mr_slam_amd.compat import voxelocc
    t = voxelocc.GPUTransformer(np.zeros(30, np.float32), 10, 1, 1, 120, 120, 1, 1)
    with pytest.raises(_lib.MrsError):
        t.retreive()
    from mr_slam_amd import ring
    xyz, offs = torch.zeros(30), torch.tensor([0, 10])
    for fused in (False, True):       # host tensors are rejected, not computed on
        with pytest.raises(_lib.MrsError):
            ring.ring_descriptors(xyz, offs, fused=fused)


def test_product_never_imports_oracle():
    """oracle/ is test infrastructure: no module of the package may reference it."""
    pkg = os.path.join(ROOT, "mr_slam_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".cpp", ".h")):
                txt = open(os.path.join(dp, f)).read()
                assert "pyoracle" not in txt and "liboracle" not in txt and "import oracle" not in txt, f


def _loaded():
    from mr_slam_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib, _lib.load()


def _declared_arg_counts():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrslam_hip.h")).read(), flags=re.S)
    return {n: (0 if a.strip() == "void" else a.count(",") + 1) for n, a in re.findall(r"\b(mrs_[a-z0-9_]+)\s*\(([^)]*)\)", src)}


def test_prototypes_cover_the_header():
    """The binding reads every declared function, each with its declared number of arguments."""
    from mr_slam_amd import _lib
    protos = _lib.parse_header(_lib.HEADER)
    assert sorted(protos) == _declared_symbols()
    counts = _declared_arg_counts()
    assert {n: len(p) for n, (_, p) in protos.items()} == counts
    assert set(_lib.VALUE_RETURNING) <= set(protos)


def test_status_becomes_mrs_error():
    """The C side's null check (no GPU involved) arrives as MrsError carrying the status."""
    _lib, lib = _loaded()
    with pytest.raises(_lib.MrsError) as e:
        lib.mrs_loopdb_size(None, None)
    assert e.value.status == 1 and "null pointer" in str(e.value)


def test_argument_count_is_checked():
    _lib, lib = _loaded()
    with pytest.raises(TypeError):
        lib.mrs_loopdb_size(None)
    with pytest.raises(TypeError):
        lib.mrs_loopdb_size(None, None, None)


def test_arguments_are_checked_before_the_call():
    """Each of these would fail in C with "null pointer" (ctx / handle None) if it got there."""
    import numpy as np
    import torch
    _lib, lib = _loaded()
    f32 = np.zeros(8, np.float32)
    with pytest.raises(_lib.MrsError, match="d_a.*no CPU fallback"):                        # numpy array in a d_ slot
        lib.mrs_ring_corr_fft_pairs(None, f32, None, 1, None, None, None, None)
    with pytest.raises(_lib.MrsError, match="d_b.*no CPU fallback"):                        # CPU tensor in a d_ slot
        lib.mrs_ring_corr_fft_pairs(None, None, torch.zeros(8), 1, None, None, None, None)
    with pytest.raises(TypeError, match="h_offsets"):                                       # int32 array in an int64_t* slot
        lib.mrs_gicp_batch_set_clouds_host(None, 0, f32, 3, np.zeros(2, np.int32))
    with pytest.raises(TypeError, match="out_n"):                                           # Python int in a pointer slot
        lib.mrs_loopdb_size(None, 5)
    with pytest.raises(TypeError):                                                          # float in an int32_t slot
        lib.mrs_radon_plan_set_option(None, 1.5, 1)


def test_stale_library_is_refused(tmp_path, monkeypatch):
    from mr_slam_amd import _lib
    _loaded()
    src = open(_lib.HEADER).read()
    assert "#define MRS_ABI_VERSION 1\n" in src
    hdr = tmp_path / "mrslam_hip.h"
    hdr.write_text(src.replace("#define MRS_ABI_VERSION 1\n", "#define MRS_ABI_VERSION 2\n"))
    monkeypatch.setattr(_lib, "HEADER", str(hdr))
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.MrsError, match="ABI version"):
        _lib.load()


def test_call_sites_pass_the_declared_argument_count():
    """Static check of every `.mrs_*(...)` call in the package, including paths the GPU suite does not reach."""
    import ast
    counts = _declared_arg_counts()
    checked, wrong = 0, []
    for dp, _, files in os.walk(os.path.join(ROOT, "mr_slam_amd")):
        for f in (f for f in files if f.endswith(".py")):
            path = os.path.join(dp, f)
            for node in ast.walk(ast.parse(open(path).read())):
                if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith("mrs_")
                        and not any(isinstance(a, ast.Starred) for a in node.args)):
                    checked += 1
                    if len(node.args) != counts[node.func.attr]:
                        wrong.append("%s:%d %s" % (path, node.lineno, node.func.attr))
    assert checked >= 50 and not wrong, wrong
