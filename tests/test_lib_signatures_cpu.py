"""The ctypes table in prime_amd/ops/_lib.py against the C declarations.

ctypes passes whatever the table says: an entry that disagrees with its
`PRIME_API` declaration hands the kernel launch garbage pointers without a
complaint. This parses the declarations out of the .hip sources (no
compiler, no library, no GPU) and requires the table to match them.
"""
import ctypes
import re
from pathlib import Path

from prime_amd.ops import _lib

CSRC = Path(_lib.__file__).resolve().parent / "csrc"

_DECL = re.compile(r"PRIME_API\s+([\w\s\*]+?)\s*\b(\w+)\s*\(([^()]*)\)")
_SCALARS = {"int64_t": ctypes.c_int64, "double": ctypes.c_double,
            "int": ctypes.c_int}


def _ctype_of(param: str, where: str):
    tokens = [t for t in param.replace("*", " * ").split() if t != "const"]
    if "*" in tokens or tokens[0] == "hipStream_t":
        return ctypes.c_void_p
    # "<type> <name>" or a bare "<type>"; anything longer is a type this
    # table has no rule for
    assert len(tokens) <= 2 and tokens[0] in _SCALARS, (
        f"{where}: no ctypes rule for parameter '{param}'")
    return _SCALARS[tokens[0]]


def _declarations():
    """name -> (return type, [ctypes of the parameters], file)"""
    decls = {}
    for src in sorted(CSRC.glob("*.hip")):
        text = re.sub(r"//[^\n]*", "", src.read_text())
        for ret, name, params in _DECL.findall(text):
            assert name not in decls, f"{name} declared twice"
            params = params.strip()
            plist = [] if params in ("", "void") else params.split(",")
            where = f"{src.name}:{name}"
            decls[name] = (" ".join(ret.split()),
                           [_ctype_of(p.strip(), where) for p in plist],
                           src.name)
    return decls


def test_sigs_table_matches_c_declarations():
    decls = _declarations()
    assert decls, f"no PRIME_API declarations found under {CSRC}"
    assert set(decls) == set(_lib._SIGS), (
        f"only in csrc: {sorted(set(decls) - set(_lib._SIGS))}; "
        f"only in _SIGS: {sorted(set(_lib._SIGS) - set(decls))}")
    for name, (ret, argtypes, fname) in sorted(decls.items()):
        # _load() sets restype = c_int on every entry
        assert ret == "int", f"{fname}:{name} returns '{ret}', not int"
        table = list(_lib._SIGS[name])
        assert len(table) == len(argtypes), (
            f"{name}: _SIGS has {len(table)} arguments, {fname} declares "
            f"{len(argtypes)}")
        for i, (have, want) in enumerate(zip(table, argtypes)):
            assert have is want, (
                f"{name} argument {i}: _SIGS says {have.__name__}, {fname} "
                f"declares {want.__name__}")


def test_flash_bwd_dkv_shape():
    """The one entry point whose argument list changed when the unused
    lse/delta pointers were dropped: 12 pointers (stream included), six
    sizes, the scale, ten more integers, doc_end."""
    want = ([ctypes.c_void_p] * 12 + [ctypes.c_int64] * 6 + [ctypes.c_double]
            + [ctypes.c_int64] * 10 + [ctypes.c_void_p])
    assert _declarations()["prime_flash_bwd_dkv"][1] == want
    assert "prime_attn_delta" not in _lib._SIGS
