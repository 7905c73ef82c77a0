"""CPU: the seven exports of the operator's domain (otmb_op_submatrix[_dev], otmb_op_take_values, otmb_op_fetch[_dev], otmb_op_get_lines[_dev])
are declared in include/otmb.h with the stated prototypes, mirrored in capi.SYMBOLS with matching kinds, and exported by the built library."""
from operator_calls_rec import header_names
from test_julia_shim_static import ctypes_kind, header_prototypes

WANT = {
    "otmb_op_submatrix_dev": ["parent", "nr", "rows", "nc", "cols", "out"],
    "otmb_op_submatrix": ["parent", "nr", "rows", "nc", "cols", "out"],
    "otmb_op_take_values": ["child", "parent", "parent_slot", "child_slot"],
    "otmb_op_fetch_dev": ["op", "slot", "colptr", "rowval", "nzval"],
    "otmb_op_fetch": ["op", "slot", "colptr", "rowval", "nzval"],
    "otmb_op_get_lines_dev": ["op", "next", "has_lines"],
    "otmb_op_get_lines": ["op", "next", "has_lines"],
}
KINDS = {
    "otmb_op_submatrix": ["ptr", "i64", "ptr", "i64", "ptr", "ptr"],
    "otmb_op_take_values": ["ptr", "ptr", "i64", "i64"],
    "otmb_op_fetch": ["ptr", "i64", "ptr", "ptr", "ptr"],
    "otmb_op_get_lines": ["ptr", "ptr", "ptr"],
}


def test_the_seven_exports_are_declared_mirrored_and_exported():
    from otmb_amd import capi

    protos = header_prototypes()
    lib = capi.lib()
    for name, names in WANT.items():
        assert name in protos, f"{name} is not declared in include/otmb.h"
        assert header_names(name) == names, name
        ret, args = protos[name]
        assert ret == "i32" and args == KINDS[name[:-4] if name.endswith("_dev") else name], (name, args)
        assert name in capi.SYMBOLS, f"{name} is not in capi.SYMBOLS"
        res, argtypes = capi.SYMBOLS[name]
        assert ctypes_kind(res) == [ret] and [ctypes_kind(t)[0] for t in argtypes] == args, name
        assert hasattr(lib, name), f"{name} is not exported by the library"
    # the _dev variants take the arguments of the host variants
    for name in ("otmb_op_submatrix", "otmb_op_fetch", "otmb_op_get_lines"):
        assert protos[name] == protos[name + "_dev"]
