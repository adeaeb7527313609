"""The C headers under include/ read as ctypes signatures, and the comparison that holds a binding's two tables to them.  TEST
INFRASTRUCTURE, plain importable module (no fixtures, no pytest hooks); tests/test_cabi.py runs both for every ABI unit."""
import ctypes
import os
import re

from conftest import ROOT

_CTYPE = {'sconf_stream_t': ctypes.c_void_p, 'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'int32_t': ctypes.c_int, 'float': ctypes.c_float,
          'double': ctypes.c_double}
_RESTYPE = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'const char*': ctypes.c_char_p}


def header_abi(header_file, name_prefix):
    """(name -> (argtypes, restype), enumerator -> value) of include/<header_file>.  Every statement between the extern "C" braces
    must be the stream typedef, an anonymous enum or the declaration of a `name_prefix`* function over the types above: anything
    else raises."""
    src = open(os.path.join(ROOT, 'include', header_file)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    body = re.search(r'extern "C" \{\s*#endif(.*)#ifdef __cplusplus\s*\}', src, flags=re.S).group(1)
    funcs, enums = {}, {}
    for stmt in (' '.join(s.split()) for s in body.split(';')):
        if not stmt or stmt == 'typedef struct ihipStream_t* sconf_stream_t':
            continue
        m = re.fullmatch(r'enum \{(.*)\}', stmt)
        if m:
            for item in m.group(1).split(','):
                k, v = re.fullmatch(r'\s*(SCONF_[A-Z0-9_]+) = (\d+)\s*', item).groups()
                assert k not in enums, k
                enums[k] = int(v)
            continue
        m = re.fullmatch(r'(const char\*|int64_t|int) (sconf_[a-z0-9_]+) ?\((.*)\)', stmt)
        assert m, f'include/{header_file}: cannot classify the statement {stmt!r}'
        ret, name, params = m.groups()
        assert name.startswith(name_prefix), f'include/{header_file}: {name} is not a {name_prefix}* function'
        args = []
        for p in ([] if params.strip() == 'void' else params.split(',')):
            p = p.strip()
            pm = re.fullmatch(r'(?:const )?([a-z0-9_]+) ?(\*?) ?[A-Za-z_][A-Za-z0-9_]*', p)
            assert pm and (pm.group(2) or pm.group(1) in _CTYPE), f'include/{header_file}: {name}: cannot classify the parameter {p!r}'
            args.append(ctypes.c_void_p if pm.group(2) else _CTYPE[pm.group(1)])
        assert name not in funcs, f'{name} declared twice'
        funcs[name] = (args, _RESTYPE[ret])
    return funcs, enums


def assert_binding_is_header(funcs, prototypes, plain, where):
    """`prototypes` (status-returning launchers) and `plain` (queries) of the binding module `where` declare exactly the header's
    functions, signature for signature.  (A swapped int / int64_t or a dropped argument would be a miscall into a kernel.)"""
    bound = {n: (a, ctypes.c_int) for n, a in prototypes.items()}
    assert not set(bound) & set(plain)
    bound.update(plain)
    assert set(bound) == set(funcs), set(bound) ^ set(funcs)
    for name, (args, res) in funcs.items():
        got_args, got_res = bound[name]
        assert got_res is res, f'{name}: returns {res.__name__} in the header, {got_res.__name__} in {where}'
        assert len(got_args) == len(args), f'{name}: {len(args)} arguments in the header, {len(got_args)} in {where}'
        for i, (g, w) in enumerate(zip(got_args, args)):
            assert g is w, f'{name}: argument {i} is {w.__name__} in the header, {g.__name__} in {where}'
