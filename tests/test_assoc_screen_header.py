"""CPU: the screened association's C-ABI constants agree between include/gmmloc_hip.h and gmmloc_amd.api, and its option is
listed with the others."""
import os
import re

from gmmloc_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "gmmloc_hip.h")) as f:
        return f.read()


def _enum(text, name):
    return int(re.search(r"\b%s\s*=\s*(\d+)" % name, text).group(1))


def test_screened_mode_and_counters_match_header():
    h = _header()
    assert _enum(h, "GL_ASSOC_SCREENED") == api.ASSOC_SCREENED == 3
    assert _enum(h, "GL_COUNTER_ASSOC_SCREEN_VERIFIED") == api.COUNTER_ASSOC_SCREEN_VERIFIED
    assert _enum(h, "GL_COUNTER_ASSOC_SCREEN_FALLBACK") == api.COUNTER_ASSOC_SCREEN_FALLBACK
    assert _enum(h, "GL_COUNTER_COUNT") == api.COUNTER_ASSOC_SCREEN_FALLBACK + 1


def test_screen_option_listed():
    assert "assoc_screen32" in _header()
    with open(os.path.join(ROOT, "gmmloc_amd", "csrc", "gl_api.hip")) as f:
        assert "X(assoc_screen32)" in f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "`assoc_screen32`" in f.read()
