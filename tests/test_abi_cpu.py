"""The whole C ABI, header by header (no GPU): every header of ``build.ABI_HEADERS`` lies under include/, declares exactly the names of its ``hip`` table at its
frozen count, with the table's return types, argument counts and -- where the prototype says which pointer is what -- argument types; no two headers share a
name; the product library exports and binds every product table.  What is specific to one header (citations, constants, refusals) is in its family's test."""
import os

import pytest

import abi_headers
from coalign_amd import build, hip


@pytest.mark.parametrize("header", build.ABI_HEADERS)
def test_header_table_and_library_agree(header):
    assert os.path.isfile(abi_headers.path(header))
    assert sorted(build.ABI_HEADERS) == sorted(os.listdir(build.INCLUDE))
    assert list(hip.HEADERS) + [abi_headers.LAB_HEADER] == list(build.ABI_HEADERS) and sorted(abi_headers.FROZEN) == sorted(build.ABI_HEADERS)
    table, declared = abi_headers.table(header), abi_headers.declarations(header)
    assert set(declared) == abi_headers.names(header) == set(table), set(declared) ^ set(table)
    assert len(declared) == abi_headers.FROZEN[header]
    for name, (res, args) in declared.items():
        assert table[name][0] is res and len(table[name][1]) == len(args), name
        if header in abi_headers.TYPED_BY_RULE:
            assert table[name][1] == [abi_headers.ctype(a) for a in args], name
    for other in build.ABI_HEADERS:
        assert other == header or not (set(table) & abi_headers.names(other)), (header, other)
    lib = hip.lib()
    assert lib.coalign_abi_version() == 2
    assert b"UNSUPPORTED" in lib.coalign_status_string(-3)
    if header != abi_headers.LAB_HEADER:                             # the laboratory header's names are in the laboratory library alone
        for name, (res, args) in table.items():
            fn = getattr(lib, name)                                  # AttributeError: declared and tabled, but not exported
            assert fn.restype is res and list(fn.argtypes) == args, name
