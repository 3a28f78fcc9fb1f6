"""What the album attention's host tests share -- tests/test_attn_{shared,pooled,pool}*_host.py: the library, its last
error message, and the declarations of include/fvta_hip.h.  A test module gets the fixture by importing it:
`from tests._album_attn_host import lib  # noqa: F401`."""
import os
import re

import pytest

from fvta_memexqa_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fvta_hip.h")


@pytest.fixture(scope="module")
def lib():
    """the loaded library, built first where it is absent"""
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def err(lib):
    return lib.fvta_last_error()


def header_code():
    """include/fvta_hip.h without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def declared_symbols():
    """the fvta_* functions the header declares"""
    return set(re.findall(r"\b(fvta_[a-z0-9_]+)\s*\(", header_code()))
