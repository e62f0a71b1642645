"""A small parser of include/xvec_hip.h and the check that holds the ctypes table of tf_kaldi_speaker_amd._lib to it.

parse(text) -> {name: (return type, [argument type, ...])}, the C types as normalised strings ("const float*", "int64_t").
check(table, protos) -> [(function name, what is wrong), ...] for a table of (name, restype, argtypes) entries; empty when the
table and the header agree.  Test code only: the product never reads the header.
"""
import ctypes as C
import re

# C struct of the header -> name of its ctypes mirror in _lib
MIRRORS = {"xv_model_desc": "ModelDesc", "xv_plan_info": "PlanInfo", "xv_kernel_time": "KernelTime", "xv_mfcc_opts": "MfccOpts",
           "xv_fbank_opts": "FbankOpts", "xv_reverb_utt": "ReverbUtt", "xv_reverb_noise": "ReverbNoise"}

RETURNS = {"void": None, "const char*": C.c_char_p, "int": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32}
SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double,
           "uint32_t": C.c_uint32}


_FIELD_TYPES = {C.c_int32: "int32_t", C.c_int64: "int64_t", C.c_float: "float", C.c_double: "double", C.c_char: "char"}


def _c_type(t):
    return "%s[%d]" % (_FIELD_TYPES[t._type_], t._length_) if issubclass(t, C.Array) else _FIELD_TYPES[t]


def layout_program(lib_module):
    """-> (C source, expected output lines).  The program includes the header and prints sizeof of every mirrored struct,
    offsetof of every field the mirror names and the value of every XV_* constant lib_module defines; a field the header types
    differently from the mirror fails the compile."""
    body, expect = [], []
    for struct, mirror_name in MIRRORS.items():
        mirror = getattr(lib_module, mirror_name)
        body.append('printf("%s %%zu\\n", sizeof(%s));' % (struct, struct))
        expect.append("%s %d" % (struct, C.sizeof(mirror)))
        for field, ftype in mirror._fields_:
            body.append('_Static_assert(__builtin_types_compatible_p(__typeof__(((%s*)0)->%s), %s), "%s.%s");'
                        % (struct, field, _c_type(ftype), struct, field))
            body.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (struct, field, struct, field))
            expect.append("%s.%s %d" % (struct, field, getattr(mirror, field).offset))
    for name in sorted(n for n in vars(lib_module) if n.startswith("XV_")):
        body.append('printf("%s %%d\\n", (int)%s);' % (name, name))
        expect.append("%s %d" % (name, getattr(lib_module, name)))
    src = '#include <stddef.h>\n#include <stdio.h>\n#include "xvec_hip.h"\nint main(void) {\n  %s\n  return 0;\n}\n' % "\n  ".join(body)
    return src, expect


def strip(text):
    """The header without comments, preprocessor lines, the extern "C" bracket and the bodies of structs and enums."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = "\n".join(l for l in text.split("\n") if not l.lstrip().startswith("#"))
    text = text.replace('extern "C" {', " ")
    return re.sub(r"\{[^{}]*\}", " ", text)


def _norm(ctype):
    """'const  float *x_dev' minus the parameter name -> 'const float*'."""
    return re.sub(r"\s*\*\s*", "*", " ".join(ctype.split()))


def parse(text):
    protos = {}
    for stmt in strip(text).split(";"):
        m = re.fullmatch(r"\s*([A-Za-z_][\w\s\*]*?)\s*\b(xv_[a-z0-9_]+)\s*\(([^()]*)\)\s*", stmt)
        if not m or m.group(1).split()[0] == "typedef":
            continue
        ret, name, args = _norm(m.group(1)), m.group(2), m.group(3).strip()
        assert name not in protos, "declared twice: " + name
        types = []
        if args != "void":
            for a in args.split(","):
                am = re.fullmatch(r"\s*(.*?[\s\*])([A-Za-z_]\w*)\s*", a)      # type, then the parameter's name
                assert am, "%s: cannot read parameter %r" % (name, a)
                types.append(_norm(am.group(1)))
        protos[name] = (ret, types)
    return protos


def searched_names(text):
    """Every xv_ name in front of a parenthesis, comments included: the set the parser may not fall short of."""
    return set(re.findall(r"\b(xv_[a-z0-9_]+)\s*\(", text))


def _arg_problem(ctype, have, lib_module):
    if "*" not in ctype:
        want = SCALARS.get(ctype)
        if want is None:
            return "header type %r is not one the check knows" % ctype
        return None if have is want else "header %s, table %s" % (ctype, getattr(have, "__name__", have))
    base, stars = ctype.replace("const", "").replace("*", " ").split(), ctype.count("*")
    pointee = " ".join(base)
    if have is C.c_void_p:
        return None
    if have is C.c_char_p:
        return None if pointee == "char" and stars == 1 else "c_char_p for header %s" % ctype
    if isinstance(have, type) and issubclass(have, C._Pointer):
        target = have._type_
        if stars == 2:                                    # xv_handle** out: a slot for an opaque pointer
            want = C.c_void_p
        elif pointee in MIRRORS:
            want = getattr(lib_module, MIRRORS[pointee])
        else:
            want = SCALARS.get(pointee)
        return None if want is not None and target is want else "POINTER(%s) for header %s" % (target.__name__, ctype)
    return "header %s is a pointer, table has %s" % (ctype, getattr(have, "__name__", have))


def check(table, protos, lib_module):
    """Compare (name, restype, argtypes) entries with parse()'s prototypes.  Returns [(function, message)]."""
    problems = []
    entries = {}
    for name, restype, argtypes in table:
        if name in entries:
            problems.append((name, "listed twice in the table"))
        entries[name] = (restype, tuple(argtypes))
    for name in sorted(set(protos) - set(entries)):
        problems.append((name, "declared in the header, missing from the table"))
    for name in sorted(set(entries) - set(protos)):
        problems.append((name, "in the table, not declared in the header"))
    for name in sorted(set(entries) & set(protos)):
        (ret, ctypes_), (restype, argtypes) = protos[name], entries[name]
        if ret not in RETURNS:
            problems.append((name, "return type %r is not one the check knows" % ret))
        elif restype is not RETURNS[ret]:
            problems.append((name, "returns %s in the header, %s in the table" % (ret, getattr(restype, "__name__", restype))))
        if len(ctypes_) != len(argtypes):
            problems.append((name, "%d arguments in the header, %d in the table" % (len(ctypes_), len(argtypes))))
            continue
        for i, (ctype, have) in enumerate(zip(ctypes_, argtypes)):
            msg = _arg_problem(ctype, have, lib_module)
            if msg:
                problems.append((name, "argument %d: %s" % (i, msg)))
    return problems
