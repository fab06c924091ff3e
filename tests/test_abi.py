"""CPU-side checks of the drop-in boundary: the shared library loads and exports every symbol
include/jsplayer_amd.h declares; no compute is attempted without a GPU."""
import ctypes
import os
import re

import pytest

from jsplayer_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols(headers=("jsplayer_amd.h", "jsplayer_amd_lab.h")):
    """Every jsp_* function the headers under include/ declare: the drop-in boundary and the measurement helpers beside it."""
    syms = set()
    for h in headers:
        text = open(os.path.join(ROOT, "include", h)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        syms |= set(re.findall(r"\b(jsp_[a-z0-9_]+)\s*\(", text))
    return sorted(syms)


def test_measurement_helpers_are_not_part_of_the_boundary():
    boundary = declared_symbols(("jsplayer_amd.h",))
    assert "jsp_measure_fill" not in boundary and "jsp_measure_h2d" not in boundary
    assert declared_symbols(("jsplayer_amd_lab.h",)) == ["jsp_measure_fill", "jsp_measure_h2d"]


def test_header_declares_the_ivideocodec_surface():
    syms = declared_symbols()
    for required in ["jsp_codec_create", "jsp_codec_destroy", "jsp_preinit", "jsp_previous_frame",
                     "jsp_is_key_frame", "jsp_state", "jsp_continue_i", "jsp_decompress_i",
                     "jsp_decompress_p", "jsp_needs_index"]:
        assert required in syms


def test_library_exports_every_declared_symbol():
    handle = ctypes.CDLL(N.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(handle, name), f"{name} declared in include/jsplayer_amd.h but not exported"


def test_binding_table_matches_header():
    assert sorted(N.SIGNATURES) == declared_symbols()
    assert N.lib().jsp_version().decode().startswith("jsplayer_amd")


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from jsplayer_amd import MSVideo1_16bit, CodecError
    with pytest.raises(CodecError):
        MSVideo1_16bit(16, 16)


def test_product_does_not_reference_the_oracle():
    """The shipped package must not import, link or call anything under oracle/."""
    pkg = os.path.join(ROOT, "jsplayer_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".h", ".hip", "Makefile")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert "oracle/" not in text and "liboracle" not in text and "oracle_binding" not in text, \
                    f"{f} refers to the oracle"


def test_every_environment_variable_the_library_reads_is_documented():
    """The shipped library reads exactly the environment variables INTEGRATION.md documents: the string literals passed to getenv and
    to jsp_pool.cpp's env() helper under jsplayer_amd/csrc/ and include/, against the JSP_* names in the paragraphs of INTEGRATION.md
    that speak of environment variables.  (Lab switches are not shipped: a measurement that needs one builds a variant.)"""
    read = set()
    for top in (os.path.join(ROOT, "jsplayer_amd", "csrc"), os.path.join(ROOT, "include")):
        for dirpath, _, files in os.walk(top):
            for f in files:
                if f.endswith((".cpp", ".h", ".hip")):
                    text = open(os.path.join(dirpath, f), errors="replace").read()
                    read.update(re.findall(r'\b(?:getenv|env)\(\s*"([^"]+)"', text))
    paragraphs = re.split(r"\n(?=\* |#|\s*\n)", open(os.path.join(ROOT, "INTEGRATION.md")).read())
    documented = set()
    for p in paragraphs:
        if "environment variable" in p:
            documented.update(re.findall(r"`(JSP_[A-Z0-9_]+)", p))
    assert read, "no getenv found: the scan is broken"
    assert read == documented, f"read but not documented: {sorted(read - documented)}; documented but not read: {sorted(documented - read)}"


def test_threaded_host_layers_are_clean_under_thread_sanitizer(tmp_path):
    """tools/tsan_cpu.sh: jsp_api.cpp, jsp_pool.cpp, msv1_codec.cpp, sp_codec.cpp, jsp_shard.cpp and the host stages built with -fsanitize=thread against
    the stub HIP runtime under tests/tsan/ and driven on 26 host threads (asynchronous submit / wait out of phase, drains, prefetch ranges
    given up mid-flight, staged batches, pools created and destroyed side by side).  Round 6's first run found a race — the caller's thread
    reading the stream decoder's settings while the first group's worker wrote its key-frame layout into the same decoder (sp_codec.cpp,
    `settings_at_submit`)."""
    import shutil
    import subprocess
    if not shutil.which("g++"):
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, JSP_TSAN_DIR=str(tmp_path))
    res = subprocess.run([os.path.join(root, "tools", "tsan_cpu.sh"), "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1200, env=env)
    out = res.stdout.decode()
    assert res.returncode == 0 and "tsan clean" in out, out[-3000:]
