"""CPU: libsoccdpt_hip.so loads and exports every symbol include/soccdpt_hip.h declares
(no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(REPO, "include", "soccdpt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(soccdpt_[a-z_0-9]+)\s*\(", text)))


def test_header_symbols_exported():
    so = os.path.join(REPO, "soccdpt_amd", "libsoccdpt_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(so)
    names = _declared()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/soccdpt_hip.h but not exported"
    lib.soccdpt_abi_version.restype = ctypes.c_int
    header = open(os.path.join(REPO, "include", "soccdpt_hip.h")).read()
    declared_version = int(re.search(r"#define\s+SOCCDPT_ABI_VERSION\s+(\d+)", header).group(1))
    from soccdpt_amd import lib as binding
    # one version number in three places: the header, the compiled library, the ctypes binding (it had never moved)
    assert lib.soccdpt_abi_version() == declared_version == binding.ABI_VERSION >= 3


def test_binding_struct_sizes_match_the_library():
    """The ctypes mirrors of the public structs have exactly the size the LIBRARY was compiled with (soccdpt_sizeof): a field added to
    soccdpt_igemm_args / soccdpt_config without the binding following is caught here and at load_library()."""
    from soccdpt_amd.lib import CalibOptions, CalibReport, FwdAuxArgs, IgemmArgs, KernelStat, SoccdptConfig, TrainAuxArgs, TrainLayerBwdArgs, load_library
    L = load_library()
    assert L.soccdpt_sizeof(3) == ctypes.sizeof(CalibReport)
    assert L.soccdpt_sizeof(4) == ctypes.sizeof(CalibOptions) == 20
    assert L.soccdpt_sizeof(0) == ctypes.sizeof(SoccdptConfig)
    assert L.soccdpt_sizeof(1) == ctypes.sizeof(IgemmArgs)
    assert L.soccdpt_sizeof(2) == ctypes.sizeof(KernelStat)
    assert L.soccdpt_sizeof(5) == ctypes.sizeof(TrainLayerBwdArgs) == 14 * 4 + 7 * 8
    assert L.soccdpt_sizeof(6) == ctypes.sizeof(TrainAuxArgs) == 2 * 4 + 6 * 8 + 3 * 4 + 4 + 12 * 8
    assert L.soccdpt_sizeof(7) == ctypes.sizeof(FwdAuxArgs) == 2 * 4 + 6 * 8 + 3 * 4 + 4 + 12 * 8
    assert L.soccdpt_sizeof(99) == 0


def test_binding_struct_matches_header():
    from soccdpt_amd.lib import SoccdptConfig
    # 9 int32 + 4 f32 + 3 int32 + 9 f32 + 27 f32
    assert ctypes.sizeof(SoccdptConfig) == 4 * (9 + 4 + 3 + 9 + 27)


def test_no_cpu_fallback():
    """Without a GPU the product path must raise, not fall back."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from soccdpt_amd.lib import Engine, make_config
    from oracle import soccdpt_ref as R
    cam, cfg = R.Camera(), R.ProjConfig()
    c = make_config("swin2t16_256", 3, 256, True, True, cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy,
                    cfg.grid_size, cfg.occupancy_shape(), cfg.pc_scale, cfg.pc_shift, cfg.correction_angle)
    with pytest.raises(RuntimeError):
        Engine(c, torch.device("cuda:0"))


def test_device_code_has_no_packed_f32_ops(tmp_path):
    """The shipped gfx950 code objects carry no v_pk_*_f32 instructions (soccdpt_amd/csrc/Makefile NOPK; DESIGN.md section 4:
    a kernel dense in packed-f32 math returned wrong sums when it shared CUs with another stream's MFMA kernel)."""
    import shutil
    import subprocess
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    so = os.path.join(REPO, "soccdpt_amd", "libsoccdpt_hip.so")
    if not os.path.exists(objdump) or not os.path.exists(so):
        pytest.skip("llvm-objdump or the built library is not present")
    local = str(tmp_path / "lib.so")
    shutil.copy(so, local)
    subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=str(tmp_path))
    bundles = [f for f in os.listdir(tmp_path) if f.endswith("gfx950")]
    assert bundles, "no gfx950 code object found in libsoccdpt_hip.so"
    packed = 0
    for b in bundles:
        asm = subprocess.run([objdump, "-d", str(tmp_path / b)], check=True, capture_output=True, text=True).stdout
        packed += len(re.findall(r"\bv_pk_(?:mul|add|fma)_f32\b", asm))
    assert packed == 0, f"{packed} packed-f32 instructions in the device code"


def test_gn_apply_issues_its_partial_loads_back_to_back(tmp_path):
    """gn_apply_kernel adds up to twelve per-tile GroupNorm partials per thread.  Written as `tt < tps ? part[tt] : 0` every one of them compiled to
    s_cbranch_execz / global_load / s_waitcnt vmcnt(0): nine dependent L2 round trips in a launch that is one round of workgroups long (DESIGN.md 11.5,
    4.44 -> 4.30 ms on the hybrid forward once the addresses were clamped and the select moved behind the loads).  Guard: in every gn_apply instantiation of the
    shipped code object there is a run of at least 8 global_load_dwordx2 with no branch and no s_waitcnt vmcnt(0) between them."""
    import shutil
    import subprocess
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    so = os.path.join(REPO, "soccdpt_amd", "libsoccdpt_hip.so")
    if not os.path.exists(objdump) or not os.path.exists(so):
        pytest.skip("llvm-objdump or the built library is not present")
    local = str(tmp_path / "lib.so")
    shutil.copy(so, local)
    subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=str(tmp_path))
    bundles = [f for f in os.listdir(tmp_path) if f.endswith("gfx950")]
    assert bundles
    seen = 0
    for b in bundles:
        asm = subprocess.run([objdump, "-d", "--no-show-raw-insn", str(tmp_path / b)], check=True, capture_output=True, text=True).stdout
        name, run, best = None, 0, 0
        for line in asm.splitlines() + ["0 <end>:"]:
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                if name and "gn_apply_kernel" in name:
                    seen += 1
                    assert best >= 8, (name, best)
                name, run, best = m.group(1), 0, 0
                continue
            t = line.strip()
            if t.startswith("global_load_dwordx2"):
                run += 1
                best = max(best, run)
            elif t.startswith("s_cbranch") or (t.startswith("s_waitcnt") and "vmcnt(0)" in t):
                run = 0
    assert seen >= 8, seen          # 4 output formats x pixels-per-thread variants


def test_igemm_kernels_use_no_scratch(tmp_path):
    """Every igemm_kernel instantiation must keep its descriptor and address arrays in registers: a select between two per-thread arrays
    once demoted the whole IgemmDesc to private memory in 24 instantiations (472 bytes of scratch per lane, 4-5x slower launches) without
    any functional symptom.  Checked on the shipped gfx950 code object's kernel descriptors."""
    import shutil
    import subprocess
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    so = os.path.join(REPO, "soccdpt_amd", "libsoccdpt_hip.so")
    if not os.path.exists(objdump) or not os.path.exists(readelf) or not os.path.exists(so):
        pytest.skip("llvm tools or the built library are not present")
    local = str(tmp_path / "lib.so")
    shutil.copy(so, local)
    subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=str(tmp_path))
    bundles = [f for f in os.listdir(tmp_path) if f.endswith("gfx950")]
    assert bundles
    n = 0
    for b in bundles:
        notes = subprocess.run([readelf, "--notes", str(tmp_path / b)], check=True, capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            scratch = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
            if name and scratch and "igemm_kernel" in name.group(1):
                n += 1
                assert int(scratch.group(1)) == 0, f"{name.group(1)} uses {scratch.group(1)} bytes of scratch per lane"
    assert n >= 40, f"only {n} igemm kernels found in the code object metadata"


_C_SCALARS = {"int": ("int", True, 4), "int32_t": ("int", True, 4), "uint32_t": ("int", False, 4), "long": ("int", True, ctypes.sizeof(ctypes.c_long)),
              "int64_t": ("int", True, 8), "uint64_t": ("int", False, 8), "size_t": ("int", False, ctypes.sizeof(ctypes.c_size_t)),
              "unsigned long long": ("int", False, 8), "float": ("float", True, 4), "double": ("float", True, 8)}


def _c_class(decl: str, is_param: bool):
    """'const float* dev_x' / 'size_t' -> 'pointer' | 'void' | (int | float, signed, bytes)."""
    if "*" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    if is_param and " ".join(words) not in _C_SCALARS:
        words = words[:-1]                      # the parameter's name
    t = " ".join(words)
    return "void" if t == "void" else _C_SCALARS[t]


def _ctypes_class(t):
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "pointer"
    code = t._type_
    assert code in "iIlLqQfd", f"{t}: not a pointer, integer or float"
    return ("float" if code in "fd" else "int", code in "ilqfd", ctypes.sizeof(t))


def _header_prototypes():
    text = open(os.path.join(REPO, "include", "soccdpt_hip.h")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    out = {}
    for ret, name, params in re.findall(r"^\s*([A-Za-z_][\w \*]*?[\s\*])(soccdpt_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", code, flags=re.M):
        assert name not in out, f"{name} is declared twice"
        plist = [] if params.strip() in ("", "void") else [" ".join(p.split()) for p in params.split(",")]
        out[name] = (_c_class(ret, False), [_c_class(p, True) for p in plist])
    return out


def test_prototype_table_matches_the_header():
    """soccdpt_amd.lib.PROTOTYPES (what load_library() applies to the shared object) against the prototypes of include/soccdpt_hip.h: the same set of
    names, the same number of parameters, and in every position -- the return value included -- the same class: pointer, or signed / unsigned
    integer or float of the same width.  A parameter added to the header without the binding following fails here; no built library is needed."""
    from soccdpt_amd.lib import PROTOTYPES
    header = _header_prototypes()
    assert sorted(header) == _declared() and len(header) == 90, "the prototype regex and the symbol regex disagree about what the header declares"
    assert sorted(PROTOTYPES) == sorted(header), (sorted(set(header) - set(PROTOTYPES)), sorted(set(PROTOTYPES) - set(header)))
    assert list(PROTOTYPES) == list(header), "the table follows the header's order"
    for name, (restype, argtypes) in PROTOTYPES.items():
        want_ret, want_args = header[name]
        assert isinstance(argtypes, list), f"{name}: no argtypes"
        assert _ctypes_class(restype) == want_ret, f"{name}: returns {want_ret} in the header, {restype} in the table"
        assert len(argtypes) == len(want_args), f"{name}: {len(want_args)} parameters in the header, {len(argtypes)} in the table"
        for i, (a, w) in enumerate(zip(argtypes, want_args)):
            assert _ctypes_class(a) == w, f"{name}: parameter {i} is {w} in the header, {a} in the table"


def test_op_mlp_ln_takes_merge_before_the_stream():
    """soccdpt_op_mlp_ln reaches the kernel's PatchMerging operand layout: `int merge` sits between W and the stream in the header, the table has the 17 parameters
    and op_mlp_ln hands it on (default off) -- tests/test_mlp_fused_gpu.py runs the layout through it."""
    import inspect
    from soccdpt_amd.lib import PROTOTYPES, op_mlp_ln
    text = open(os.path.join(REPO, "include", "soccdpt_hip.h")).read()
    params = re.search(r"int\s+soccdpt_op_mlp_ln\s*\(([^)]*)\)\s*;", text).group(1)
    names = [" ".join(p.split()) for p in params.split(",")]
    assert len(names) == 17 and names[-6:] == ["int M", "int C", "int H", "int W", "int merge", "void* stream"], names[-6:]
    restype, argtypes = PROTOTYPES["soccdpt_op_mlp_ln"]
    assert restype is ctypes.c_int and len(argtypes) == 17 and argtypes[10:16] == [ctypes.c_int] * 6 and argtypes[16] is ctypes.c_void_p
    assert inspect.signature(op_mlp_ln).parameters["merge"].default is False


def test_load_library_leaves_no_function_on_ctypes_defaults():
    from soccdpt_amd.lib import PROTOTYPES, load_library
    L = load_library()
    for name, (restype, argtypes) in PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
