"""ss_attn_decode_step / ss_attn_decode_kv8_step (include/seedstory_hip.h): declared, exported, and every argument rule refused
with SS_EINVAL BEFORE anything is launched — so the refusals can be shown without a device, on pointers that are never followed.
(The launches themselves: tests/test_decode_step_gpu.py.)"""
import os

from seedstory import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, HD, CAP = 4, 64, 32
PLANE = H * CAP * HD
BF16, F32 = _lib.SS_BF16, _lib.SS_F32


def call(shadow, dtype=BF16, nb=2, hd=HD, stride=PLANE, null=None, odd=None, kv_word=0, pos_word=1):
    """the entry point on fake, 256-byte aligned addresses; `null`: that pointer argument is NULL, `odd`: it is 2 (scales: 1) bytes
    off.  -> (return code, last error)"""
    names = ["qkv", "kcache", "vcache"] + (["k_codes", "v_codes", "k_scale", "v_scale"] if shadow else []) + ["cos", "sin", "out", "ws", "state"]
    ptr = {n: 0x10000 + 0x100 * i for i, n in enumerate(names)}
    if null:
        ptr[null] = None
    if odd:
        ptr[odd] += 1 if odd.endswith("scale") else 2
    fn = lib().ss_attn_decode_kv8_step if shadow else lib().ss_attn_decode_step
    rc = fn(*[ptr[n] for n in names], kv_word, pos_word, 3, 8, nb, H, hd, CAP, stride, dtype, None)
    return rc, lib().ss_last_error()


def lib():
    return _lib.lib()


def test_abi_declares_and_exports_the_decode_step():
    with open(os.path.join(ROOT, "include", "seedstory_hip.h")) as f:
        header = f.read()
    assert "#define SS_ABI_VERSION 1" in header and lib().ss_abi_version() == 1
    for name in ("ss_attn_decode_step", "ss_attn_decode_kv8_step"):
        assert name + "(" in header and name in _lib.PROTOTYPES and getattr(lib(), name)


def test_decode_step_refusals_come_before_any_launch():
    for shadow in (False, True):
        who = b"attn_decode_kv8_step" if shadow else b"attn_decode_step"
        for kw in (dict(nb=0), dict(nb=9), dict(stride=PLANE - HD), dict(stride=PLANE + 8), dict(kv_word=-1), dict(pos_word=-1),
                   dict(odd="qkv"), dict(odd="kcache"), dict(odd="vcache"), dict(odd="cos"), dict(odd="sin"),
                   dict(null="qkv"), dict(null="vcache"), dict(null="out"), dict(null="ws"), dict(null="state")):
            rc, err = call(shadow, **kw)
            assert rc == -1 and who in err, (shadow, kw, rc, err)
        rc, err = call(shadow, hd=104, stride=H * CAP * 104)
        assert rc == -1 and b"head_dim 104" in err, (shadow, rc, err)
    for kw in (dict(dtype=F32), dict(hd=48, stride=H * CAP * 48), dict(odd="k_codes"), dict(odd="v_codes"), dict(odd="k_scale"),
               dict(odd="v_scale"), dict(null="k_codes"), dict(null="v_scale")):
        rc, err = call(True, **kw)
        assert rc == -1 and b"attn_decode_kv8_step" in err, (kw, rc, err)
