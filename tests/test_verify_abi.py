"""ZD_F_VERIFY_CHECKSUM on the host side (include/zd.h): the flag and the
status code in the header, their names in the library and in _lib, the new
entry point exported and bound, the ABI version unchanged, and the CLI's
--verify option.  No GPU: nothing here launches anything."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zd.h")).read()


def test_header_defines_the_flag_and_the_code():
    assert re.search(r"^#define\s+ZD_F_VERIFY_CHECKSUM\s+1024u\b", HEADER, re.M)
    assert re.search(r"^#define\s+ZD_E_CHECKSUM_WRONG\s+\(-100\)", HEADER, re.M)
    assert re.search(r"^#define\s+ZD_ABI_VERSION\s+8\b", HEADER, re.M)
    assert re.search(r"int\s+zd_batch_device_checksums\(const zd_batch\*\s*\w*,\s*const uint64_t\*\*\s*d_hash,"
                     r"\s*const int8_t\*\*\s*d_ok\);", HEADER)


def test_status_name_and_abi_version():
    from zstd_decompressor import _lib
    assert _lib.status_name(-100) == "ChecksumWrong"
    assert _lib.lib().zd_abi_version() == 8


def test_lib_constants():
    from zstd_decompressor import _lib
    assert _lib.F_VERIFY_CHECKSUM == 1024 and _lib.CHECKSUM_WRONG == -100
    # no other plan flag shares the bit
    others = [v for k, v in vars(_lib).items() if k.startswith("F_") and k != "F_VERIFY_CHECKSUM"]
    assert all(isinstance(v, int) and not v & _lib.F_VERIFY_CHECKSUM for v in others)


def test_symbol_exported_and_bound():
    from zstd_decompressor import _lib
    assert "zd_batch_device_checksums" in _lib.SIGNATURES
    fn = _lib.lib().zd_batch_device_checksums
    assert fn.restype is C.c_int and len(fn.argtypes) == 3


def test_null_batch_is_invalid_arg():
    from zstd_decompressor import _lib
    h, ok = C.c_void_p(), C.c_void_p()
    assert _lib.lib().zd_batch_device_checksums(None, C.byref(h), C.byref(ok)) == _lib.INVALID_ARG
    assert _lib.lib().zd_batch_device_checksums(None, None, None) == _lib.INVALID_ARG


def test_cli_parses_verify():
    from zstd_decompressor.__main__ import _parser
    assert _parser().parse_args(["x.zst", "--verify"]).verify is True
    a = _parser().parse_args(["x.zst", "--check-checksums"])
    assert a.verify is False and a.check_checksums is True


def test_python_entry_points_take_the_keyword():
    import inspect
    from zstd_decompressor import batch
    assert inspect.signature(batch.decompress).parameters["verify"].default is False
    assert callable(batch.Batch.device_checksums)
