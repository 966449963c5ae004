"""CPU-only: every struct and every prototype of include/vslnet_hip.h against its statement in vslnet_amd/abi.py.

Structs: field names in order, sizeof and every offsetof as the host C compiler lays the header out, against the ctypes mirror of the same name
(a struct without a mirror fails), and the sizes pinned at ABI 9 so that none moves unnoticed.  Prototypes: the number of parameters and the
return type of every declared function against abi.PROTOTYPES.  The feature tests keep their own facts (their symbols are exported, the fields a
feature appended, the sizes of the commit it was added to); what they share -- "the mirror is the header" -- is asserted here, once, for all."""
import ctypes
import re

import pytest

from tests.helpers import header_layout, header_source, header_structs
from vslnet_amd import abi, engine

# sizeof at ABI 9 (x86-64 / LP64: 8-byte pointers aligned at 8)
SIZEOF_AT_ABI_9 = {
    'vsl_config': 44, 'vsl_io': 208, 'vsl_loss_io': 72, 'vsl_encode_io': 56, 'vsl_localize_io': 128, 'vsl_encode_query_io': 80, 'vsl_pairs_io': 112,
    'vsl_highlight_io': 128, 'vsl_select_io': 48, 'vsl_shared_io': 24, 'vsl_group_loss_io': 176, 'vsl_topk_io': 88, 'vsl_merge_io': 136,
    'vsl_encode_windows_io': 80, 'vsl_merge_windows_io': 128, 'vsl_adamw': 36, 'vsl_fused_step': 72}
RESTYPE = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64, 'const char*': ctypes.c_char_p}


def test_the_header_declares_exactly_the_pinned_structs():
    assert sorted(header_structs()) == sorted(SIZEOF_AT_ABI_9) and len(SIZEOF_AT_ABI_9) == 17


@pytest.mark.parametrize('struct', sorted(SIZEOF_AT_ABI_9))
def test_struct_layout_matches_the_header(struct):
    size, offsets = header_layout()[struct]
    mirror = getattr(abi, struct, None)
    assert mirror is not None and issubclass(mirror, ctypes.Structure), 'no ctypes mirror of ' + struct
    assert getattr(engine, struct) is mirror                        # (tests and tools import the mirrors from vslnet_amd.engine)
    assert [f[0] for f in mirror._fields_] == header_structs()[struct]
    assert ctypes.sizeof(mirror) == size == SIZEOF_AT_ABI_9[struct]
    assert {name: getattr(mirror, name).offset for name, _ in mirror._fields_} == offsets


def test_vsl_io_ends_with_inference_and_the_version_is_9_everywhere():
    from vslnet_amd import build
    assert header_structs()['vsl_io'][-1] == 'inference'            # new fields are appended: an older build never reads behind its own last one
    assert re.search(r'#define\s+VSL_ABI_VERSION\s+9\b', header_source())
    assert ctypes.CDLL(build.build()).vsl_abi_version() == 9 == abi.ABI_VERSION == engine.ABI_VERSION


def _declared_functions():
    """{name: (return type, number of parameters)} of every function the header declares"""
    out = {}
    for ret, name, params in re.findall(r'^\s*((?:const\s+)?\w+\s*\*?)\s*(vsl_[a-z_]+)\s*\(([^)]*)\)\s*;', header_source(), flags=re.M):
        out[name] = (re.sub(r'\s*\*', '*', ' '.join(ret.split())), 0 if params.strip() == 'void' else len(params.split(',')))
    return out


def test_prototypes_match_the_declarations():
    declared = _declared_functions()
    assert sorted(declared) == sorted(abi.PROTOTYPES) == sorted(engine.ABI_SYMBOLS) and len(declared) == 43
    for name, (ret, nparams) in declared.items():
        argtypes, restype = abi.PROTOTYPES[name]
        assert len(argtypes) == nparams, (name, nparams, argtypes)
        assert restype is RESTYPE[ret], (name, ret, restype)


def test_every_feature_names_declared_symbols_and_its_refusal_names_them():
    for flag, (symbols, refusal) in abi.FEATURES.items():
        assert symbols and set(symbols) <= set(abi.PROTOTYPES), flag
        assert re.search(r'\((vsl_\w+)( / vsl_\w+)* (is|are) missing\)$', refusal), (flag, refusal)
        assert set(re.findall(r'vsl_\w+', refusal)) <= set(symbols), (flag, refusal)
