"""CPU: the C-ABI library loads and exports every symbol include/loft_hip.h declares, and every function of it is bound with
the prototype the header gives (bonai_amd.lib.prototypes): a wrong count, type or width of an argument fails at the call."""
import ast
import ctypes
import glob
import os
import re

import torch  # noqa: F401  (load torch's HIP runtime before libloft_hip.so)

from bonai_amd import lib as L


def test_header_symbols_exported():
    names = L.exported_symbols()
    assert len(names) >= 5
    if not (os.path.exists(L._LIB_PATH) and os.path.exists(L._LIB_PATH_F16)):
        from bonai_amd import build
        build.build()
    for path, code in ((L._LIB_PATH, L.BF16), (L._LIB_PATH_F16, L.F16)):      # the bfloat16 and the binary16 build: same C-ABI
        cdll = ctypes.CDLL(path)
        missing = [n for n in names if not hasattr(cdll, n)]
        assert not missing, f'symbols declared in include/loft_hip.h but not exported by {path}: {missing}'
        assert cdll.loft_act16_dtype() == code


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, I, Q, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float


def _header():
    text = open(os.path.join(ROOT, 'include', 'loft_hip.h')).read()
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def _libraries():
    if not (os.path.exists(L._LIB_PATH) and os.path.exists(L._LIB_PATH_F16)):
        from bonai_amd import build
        build.build()
    return [L.load_for(torch.bfloat16), L.load_for(torch.float16)]


def test_prototypes_drop_no_declaration():
    hdr, protos = _header(), L.prototypes()
    names = set(re.findall(r'\b(loft_[a-z0-9_]+)\s*\(', hdr))                       # the name scan exported_symbols() used to be
    assert len(names) >= 112 and set(protos) == names, sorted(names ^ set(protos))
    assert L.exported_symbols() == sorted(names)
    wide = len(re.findall(r'\bint64_t\s+loft_', hdr))
    assert wide >= 5 and sum(1 for restype, _ in protos.values() if restype is Q) == wide
    assert all(restype in (I, Q) for restype, _ in protos.values())


def test_prototypes_match_hand_written_ones():
    """The parser is not its own oracle: six declarations transcribed by hand from include/loft_hip.h."""
    want = {
        'loft_act16_dtype': (I, []),
        'loft_nms_workspace_bytes': (Q, [Q, Q, Q]),
        # keys_in, keys_out, vals_in, vals_out, int64 num_items, int num_segments, seg_offsets, workspace, workspace_bytes, stream
        'loft_segmented_sort_desc': (I, [V, V, V, V, Q, I, V, V, V, V]),
        # src wgt bias residual relu_mask out zero_page | B IH IW Cin Cout OH OW OHf OWf os oo_y oo_x ss T | dy dx wt |
        # relu out_f32 accumulate groups | src_gs wgt_gs out_gs bias_gs (int64) | variant | stream
        'loft_conv_tap_bf16_v': (I, [V] * 7 + [I] * 14 + [V] * 3 + [I] * 4 + [Q] * 4 + [I, V]),
        # a_in w1 bias1 res mask1 mid w2 bias2 mask2 out2 | int64 M | P C variant | stream
        'loft_bneck_pair_bf16_v': (I, [V] * 10 + [Q, I, I, I, V]),
        # p g m | int64 n | gnorm_sq | max_norm lr momentum weight_decay inv_world | state stream
        'loft_sgd_momentum_scaled_f32': (I, [V, V, V, Q, V, F, F, F, F, F, V, V]),
    }
    protos = L.prototypes()
    for name, proto in want.items():
        assert protos[name] == proto, name
    tap = protos['loft_conv_tap_bf16_v'][1]
    assert len(tap) == 34 and tap[28:32] == [Q] * 4 and protos['loft_bneck_pair_bf16_v'][1][10] is Q


def test_unknown_type_spelling_is_not_guessed(monkeypatch, tmp_path):
    import pytest
    hdr = tmp_path / 'loft_hip.h'
    hdr.write_text('int loft_fine(const float* x, int64_t n);\nint loft_odd(unsigned n, void* stream);\n')
    monkeypatch.setattr(L, '_HEADER', str(hdr))
    monkeypatch.setattr(L, '_prototypes', None)
    with pytest.raises(L.LoftHipError, match='loft_odd'):
        L.prototypes()


def test_both_libraries_are_typed():
    protos = L.prototypes()
    for lib in _libraries():
        for name, (restype, argtypes) in protos.items():
            fn = getattr(lib, name)
            assert fn.restype is restype and list(fn.argtypes) == argtypes and len(fn.argtypes) == len(argtypes), name


def test_misuse_is_caught_at_the_call():
    """loft_conv_wgrad_form and loft_nms_workspace_bytes touch no device."""
    import pytest
    from bonai_amd import kernels as K
    taps = [(0, 0, r - 1, s - 1, r * 3 + s) for r in range(3) for s in range(3)]
    A = [L.arr(ctypes.c_int, [t[i] for t in taps]) for i in range(5)]
    args = [1, 3, 32, 128, 3, 32, 128, 3, 32, 1, 1, 9, *A, 1, 0, K.WGRAD_AUTO]      # tests/test_wgrad_forms_cpu.py: 'ring_same_w32'
    for lib in _libraries():
        assert lib.loft_conv_wgrad_form(*args) == K.WGRAD_FORM_RING_SAME
        assert lib.loft_conv_wgrad_form(*[ctypes.c_int(a) if isinstance(a, int) else a for a in args]) == K.WGRAD_FORM_RING_SAME
        with pytest.raises(TypeError):
            lib.loft_conv_wgrad_form(*args[:-1])
        with pytest.raises(ctypes.ArgumentError):
            lib.loft_conv_wgrad_form(1.0, *args[1:])
        with pytest.raises(ctypes.ArgumentError):
            lib.loft_conv_wgrad_form(*args[:17], A[0], *args[18:])                  # an array where `groups` goes
        assert lib.loft_nms_workspace_bytes(2 ** 33, 1, 1) >= 2 ** 33               # 64-bit argument and return value survive


def _loft_calls():
    for d in ('bonai_amd', 'tools'):
        for path in sorted(glob.glob(os.path.join(ROOT, d, '**', '*.py'), recursive=True)):
            for node in ast.walk(ast.parse(open(path).read(), path)):
                if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith('loft_'):
                    yield f'{os.path.relpath(path, ROOT)}:{node.lineno} {node.func.attr}', node


def test_call_sites_match_the_header():
    """Every `<library>.loft_*(...)` call under bonai_amd/ and tools/ names a declared function and passes exactly its number of
    positional arguments -- also the call sites the GPU tests reach only in rare modes."""
    protos, checked, bad = L.prototypes(), 0, []
    for where, node in _loft_calls():
        if node.func.attr not in protos:
            bad.append(f'{where}: not declared in include/loft_hip.h')
        elif node.keywords:
            bad.append(f'{where}: keyword arguments')
        elif not any(isinstance(a, ast.Starred) for a in node.args):
            checked += 1
            if len(node.args) != len(protos[node.func.attr][1]):
                bad.append(f'{where}: {len(node.args)} arguments, declared with {len(protos[node.func.attr][1])}')
    assert not bad, '\n'.join(bad)
    assert checked >= 100, checked


def test_kernels_wrap_no_scalar_by_hand():
    """bonai_amd/kernels.py passes plain Python numbers: the prototypes convert them.  What remains of ctypes there is host arrays
    (L.arr(c_int, ...), `(c_void_p * n)(...)`) and the one out-parameter, `nbytes = c_int64(0)` of segmented_sort_desc."""
    path = os.path.join(ROOT, 'bonai_amd', 'kernels.py')
    scalar = {'c_int', 'c_int64', 'c_uint64', 'c_float', 'c_double', 'c_long', 'c_size_t'}
    made = [n for n in ast.walk(ast.parse(open(path).read())) if isinstance(n, ast.Call)
            and (n.func.id if isinstance(n.func, ast.Name) else n.func.attr if isinstance(n.func, ast.Attribute) else '') in scalar]
    in_args = {id(a) for _, node in _loft_calls() for a in ast.walk(node) if a is not node}
    assert not [n.lineno for n in made if id(n) in in_args]
    assert [ast.unparse(n) for n in made] == ['c_int64(0)'], [f'{n.lineno}: {ast.unparse(n)}' for n in made]


def test_act16_mode_switch():
    import pytest
    assert L.act16() == torch.bfloat16
    prev = L.set_act16(torch.float16)
    try:
        assert prev == torch.bfloat16 and L.act16() == torch.float16
        assert L.load().loft_act16_dtype() == L.F16
    finally:
        L.set_act16(prev)
    assert L.load().loft_act16_dtype() == L.BF16
    with pytest.raises(L.LoftHipError):
        L.set_act16(torch.float32)


def test_no_cpu_fallback():
    import pytest
    import torch
    from bonai_amd import kernels as K
    rois = torch.zeros(1, 5)
    feat = torch.zeros(1, 4, 8, 8).contiguous(memory_format=torch.channels_last)
    with pytest.raises(L.LoftHipError):
        K.roi_align_fwd([feat], rois, 7, [4])


def test_library_sources_read_no_environment():
    """The kernel library takes its variants as explicit arguments (the *_v entry points of include/loft_hip.h): no getenv in csrc."""
    import glob
    csrc = os.path.join(os.path.dirname(os.path.abspath(L.__file__)), 'csrc')
    offenders = [f for f in glob.glob(os.path.join(csrc, '*.hip')) + glob.glob(os.path.join(csrc, '*.h')) if 'getenv' in open(f).read()]
    assert not offenders, offenders


def test_selector_constants_match_the_header():
    """bonai_amd.kernels mirrors the kernel selectors of include/loft_hip.h (LOFT_CONV_* / LOFT_WGRAD_* / LOFT_ROI_* / LOFT_F32_*
    and the LOFT_CONV_FLAG_* bits) as plain integers: every mirrored name must carry the header's value."""
    import re
    from bonai_amd import kernels as K
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'loft_hip.h')).read()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r'^#define\s+(LOFT_[A-Z0-9_x]+)\s+(0x[0-9a-fA-F]+|\d+)\b', hdr, re.M)}
    checked = 0
    for name, value in defs.items():
        for prefix in ('LOFT_CONV_', 'LOFT_WGRAD_', 'LOFT_ROI_', 'LOFT_F32_'):
            if name.startswith(prefix):
                py = name[len('LOFT_'):]
                if hasattr(K, py):
                    assert getattr(K, py) == value, (name, value, getattr(K, py))
                    checked += 1
    assert checked >= 30, checked
    for must in ('F32_SPLIT6', 'F32_SPLIT3', 'F32_EXACT', 'ROI_FWD_SEP4', 'ROI_BWD_PIPE', 'CONV_STREAM256N'):
        assert 'LOFT_' + must in defs and getattr(K, must) == defs['LOFT_' + must], must
