"""The ctypes binding is derived from include/mas_hip.h (mas_hip/_header.py).  These checks pin the derivation from outside it:
hand-written signatures of the prototypes that exercise every type rule, the inputs the parser must refuse, the constants against
the header's text read by another route, the ten struct mirrors against the C compiler's own sizeof / offsetof, and the strict load."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

import mas_hip
from mas_hip import _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mas_hip.h")

p, i, f, d, ll, sz = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_longlong, C.c_size_t
Conv, Img, Row, Feats = (C.POINTER(t) for t in (mas_hip.ConvDesc, mas_hip.FaceImage, mas_hip.FaceRow, mas_hip.FaceFeats))
EXPECTED = {
    "mas_last_error": (C.c_char_p, []),
    "mas_packed_weight_elems": (sz, [i, i, i]),
    "mas_adam_blocks": (i, [ll]),
    "mas_adam_multi": (i, [p, i, i, f, f, f, f, f, d, d, p]),
    "mas_attn_decode_dev": (i, [p, p, p, ll, p, p, i, ll, i, p, ll, i, i, i, i, p, f, p]),
    "mas_token_ce_fwd": (i, [p, i, ll, i, ll, ll, ll, p, ll, f, p, p, p]),
    "mas_sample_tokens_prompt": (i, [p, ll, ll, i, i, i, i, i, p, p, p, i, p, ll, p, ll, p, ll, p, ll, p]),
    "mas_conv_fwd": (i, [Conv, p, p, p, p, p, p, p]),
    "mas_face_crop_fwd": (i, [Img, Img, Row, i, p, i, p]),
    "mas_face_l1_bwd": (i, [Feats, i, i, p, C.POINTER(p), p]),
    "mas_pack_conv_weight_batch": (i, [p, i, i, p]),          # MasPackItem*: a device table
    "mas_gn_stats": (i, [p, i, i, i, i, i, f, p, p, p, p, p, sz, p]),
    "mas_obj_canvas_fwd": (i, [Img, Img, C.POINTER(mas_hip.ObjPlan), p, p, p, i, p]),
    "mas_seg_agreement": (i, [p, p, p, i, i, i, i, i, p, p]),   # unsigned char*, int*, long long*: plain pointers
}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_derived_signature_is_the_hand_written_one(name):
    assert mas_hip._SIGNATURES[name] == EXPECTED[name]
    assert len(EXPECTED["mas_attn_decode_dev"][1]) == 18 and len(EXPECTED["mas_sample_tokens_prompt"][1]) == 21


def test_signatures_follow_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"\b(mas_[a-z0-9_]+)\s*\(", text)
    assert list(mas_hip._SIGNATURES) == names == list(mas_hip.EXPORTS) and len(names) >= 125      # every prototype, in header order
    for name, (res, args) in mas_hip._SIGNATURES.items():
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)[1]
        assert len(args) == (0 if proto.strip() == "void" else proto.count(",") + 1), name
        assert res in (i, sz, C.c_char_p), name


@pytest.mark.parametrize("text", [
    "int mas_x(unsigned short a);",              # a scalar type outside the list
    "int mas_x(long a);",
    "int mas_x(int (*callback)(int));",          # a function pointer
    "int mas_x(void*** a);",
    "int mas_x(int);",                           # a parameter without a name: `long long` would read as `long` named `long`
    "int mas_x(int a[4]);",
    "int mas_x(int a, ...);",
    "void mas_x(int a);",
    "int mas_x(int a) int mas_y(int b);",        # one prototype per `;`
    "int mas_x(int a)",
    "int other(int a);",
    "int mas_x(int a); int mas_x(float a);",
    "enum { MAS_A, MAS_B };",                    # an enumerator whose value the parser would have to count
])
def test_parser_refuses_what_it_cannot_read(text):
    with pytest.raises(ValueError, match="mas_hip.h"):
        _header.parse(text, {})


def test_parser_reads_comments_and_constants():
    text = """
    /* int mas_gone(int a); */
    // int mas_gone_too(int a);
    #ifndef MAS_GUARD_H
    #define MAS_GUARD_H
    #define MAS_N 32
    #define MAS_F(C) (8192 / (C))
    enum { MAS_A = 0,   /* first */
           MAS_B = -2   /* second */ };
    typedef struct MasS { int32_t a; void* p[4]; } MasS;
    const char* mas_a(void);
    size_t mas_b(const MasS* s, const MasOther* table, void* const* seeds,
                 long long n, int64_t* out);
    #endif
    """
    class S(C.Structure):
        _fields_ = [("a", C.c_int32), ("p", C.c_void_p * 4)]
    sigs, consts = _header.parse(text, {"MasS": S})
    assert sigs == {"mas_a": (C.c_char_p, []), "mas_b": (sz, [C.POINTER(S), p, C.POINTER(p), ll, p])}
    assert consts == {"MAS_N": 32, "MAS_A": 0, "MAS_B": -2}


def test_constants_are_the_headers():
    """read here with two regular expressions over the raw text, not by the parser under test"""
    raw = open(HEADER).read()
    want = {k: int(v) for k, v in re.findall(r"^#define\s+(MAS_\w+)\s+(-?\d+)\s*$", raw, re.M)}
    for body in re.findall(r"\benum\s*\{(.*?)\}\s*;", raw, re.S):
        want.update((k, int(v)) for k, v in re.findall(r"\b(MAS_\w+)\s*=\s*(-?\d+)", body))
    assert want == mas_hip.constants and len(want) >= 28
    assert want["MAS_ABI_VERSION"] == mas_hip.ABI_VERSION == 10 and want["MAS_ACT_AFFINE_SILU"] == 2 and want["MAS_EWORKSPACE"] == -4
    for name, value in want.items():
        assert getattr(mas_hip, name[4:]) == value, name
    for public in ("F32 BF16 ACT_NONE ACT_AFFINE ACT_AFFINE_SILU ABI_VERSION WLAYOUT_K64 WLAYOUT_K32 WLAYOUT_UP2 ATTN_DECODE_MAX_SPLITS "
                   "CE_NONE CE_MEAN CE_SUM SEG_NCHW SEG_NHWC SEG_U8 SEG_LABELS_TILE SEG_MAX_PLANES").split():
        assert getattr(mas_hip, public) == want["MAS_" + public]
    from mas_hip import face, objects, ops, seglabels
    assert seglabels.MAX_PLANES == want["MAS_SEG_MAX_PLANES"] and face.FACE == want["MAS_FACE_SIZE"]
    assert (objects.ALIGN, objects.MIN_SIDE, objects.CP) == (want["MAS_OBJ_ALIGN"], want["MAS_OBJ_MIN_SIDE"], want["MAS_OBJ_CANVAS_C"])
    assert face.MAX_ROWS == 6 and want["MAS_FACE_MAX_ROWS"] == 8                   # the reference's faces[:6] is policy, not the ABI's bound
    assert ops._DT == mas_hip._DT and all(getattr(ops, n) is getattr(mas_hip, n) for n in ("_ptr", "_stream", "_require_cuda"))


def _host_cc():
    from mas_hip import build
    cands = [shutil.which("cc")]
    try:
        rocm_bin = os.path.dirname(os.path.realpath(build._hipcc()))
        cands += [os.path.join(rocm_bin, rel) for rel in ("amdclang", "clang", "../lib/llvm/bin/clang", "../llvm/bin/clang")]
    except RuntimeError:
        pass
    return next((c for c in cands if c and os.path.exists(c)), None)


MIRRORS = ("ConvDesc", "PackItem", "PackTileItem", "AdamItem", "FaceRow", "FaceImage", "FaceBnItem", "FaceFeats", "ObjCell", "ObjPlan")


def test_struct_mirrors_have_the_compilers_layout(tmp_path):
    """sizeof, and offsetof + size of every field, of all ten mirrors; the fields must also fill the C struct, so a member the header
    has and the mirror lacks shows even where the tail padding would hide it from sizeof"""
    cc = _host_cc()
    if cc is None:
        pytest.skip("no host C compiler")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "mas_hip.h"', "int main(void) {"]
    want = []
    for name in MIRRORS:
        mirror = getattr(mas_hip, name)
        lines.append(f'    printf("{name} %zu\\n", sizeof(Mas{name}));')
        want.append(f"{name} {C.sizeof(mirror)}")
        for field, _ in mirror._fields_:
            lines.append(f'    printf("{name}.{field} %zu %zu\\n", offsetof(Mas{name}, {field}), sizeof(((Mas{name}*)0)->{field}));')
            want.append(f"{name}.{field} {getattr(mirror, field).offset} {getattr(mirror, field).size}")
        assert sum(getattr(mirror, field).size for field, _ in mirror._fields_) == C.sizeof(mirror), f"{name}: a hole no pad_ names"
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True, timeout=120)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")[:-1]
    assert got == want
    assert len(want) == len(MIRRORS) + 96 and "ConvDesc.wgrad_cus 64 4" in want and "FaceImage.sn 32 8" in want and "ObjPlan 56" in want


def test_every_struct_of_the_header_has_a_mirror():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(re.findall(r"\}\s*Mas(\w+)\s*;", text)) == sorted(MIRRORS)


def test_lib_refuses_a_library_without_a_declared_symbol(tmp_path):
    cc = _host_cc()
    if cc is None:
        pytest.skip("no host C compiler")
    src, so = tmp_path / "partial.c", tmp_path / "libpartial.so"
    src.write_text("int mas_abi_version(void) { return 10; }\nconst char* mas_last_error(void) { return \"\"; }\n")
    subprocess.run([cc, "-shared", "-fPIC", str(src), "-o", str(so)], check=True, capture_output=True, text=True, timeout=120)
    code = ("import sys; sys.path.insert(0, %r)\nimport mas_hip\ntry:\n    mas_hip.lib()\nexcept RuntimeError as e:\n    print('REFUSED', e)\n"
            % os.path.join(ROOT, "make-a-scene_amd"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MAS_HIP_LIB=str(so)), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "REFUSED" in r.stdout and "mas_last_kernel" in r.stdout and str(so) in r.stdout, r.stdout + r.stderr
