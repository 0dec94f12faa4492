"""Per-kernel static resources of the built library, read from its gfx950 code objects' own
metadata (the NT_AMDGPU_METADATA note: registers, spills, scratch, LDS) and symbol tables (code bytes).
Counts only — no instruction is read.

usage: python tools/kernel_resources.py [libisaklm_rt.so] [kernel-name-substring ...]
prints one JSON object per matching kernel (default: wf_finish_bvh and wf_long).

As a module: kernels(lib_path) -> {mangled name: {"sgpr_count", "sgpr_spill_count", "vgpr_count",
"vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size", "kernarg_segment_size",
"code_bytes", "args": [[offset, size] of each explicit argument]}}; find(lib_path, *substrings) -> the one kernel whose mangled name holds them all.
"""
import json
import os
import struct
import sys

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(os.path.dirname(HERE), "isaklm-raytracer_amd", "libisaklm_rt.so")
FIN_DEFAULT = ("wf_finish_bvh", "ILb0ELi4E")  # wf_finish_bvh<false, 4>: the flagship call's kernel


def _unpack(b, i):
    """one msgpack value at b[i:] -> (value, next index); the subset code-object metadata uses"""
    t = b[i]
    if t <= 0x7F:
        return t, i + 1
    if 0x80 <= t <= 0x8F:
        return _map(b, i + 1, t & 0x0F)
    if 0x90 <= t <= 0x9F:
        return _arr(b, i + 1, t & 0x0F)
    if 0xA0 <= t <= 0xBF:
        n = t & 0x1F
        return b[i + 1:i + 1 + n].decode(), i + 1 + n
    if t >= 0xE0:
        return t - 256, i + 1
    if t == 0xC0:
        return None, i + 1
    if t in (0xC2, 0xC3):
        return t == 0xC3, i + 1
    if t in (0xC4, 0xC5, 0xC6, 0xD9, 0xDA, 0xDB):
        w = {0xC4: 1, 0xC5: 2, 0xC6: 4, 0xD9: 1, 0xDA: 2, 0xDB: 4}[t]
        n = int.from_bytes(b[i + 1:i + 1 + w], "big")
        raw = b[i + 1 + w:i + 1 + w + n]
        return (raw if t <= 0xC6 else raw.decode()), i + 1 + w + n
    if t == 0xCA:
        return struct.unpack(">f", b[i + 1:i + 5])[0], i + 5
    if t == 0xCB:
        return struct.unpack(">d", b[i + 1:i + 9])[0], i + 9
    if 0xCC <= t <= 0xCF:
        w = 1 << (t - 0xCC)
        return int.from_bytes(b[i + 1:i + 1 + w], "big"), i + 1 + w
    if 0xD0 <= t <= 0xD3:
        w = 1 << (t - 0xD0)
        return int.from_bytes(b[i + 1:i + 1 + w], "big", signed=True), i + 1 + w
    if t in (0xDC, 0xDD):
        w = 2 if t == 0xDC else 4
        return _arr(b, i + 1 + w, int.from_bytes(b[i + 1:i + 1 + w], "big"))
    if t in (0xDE, 0xDF):
        w = 2 if t == 0xDE else 4
        return _map(b, i + 1 + w, int.from_bytes(b[i + 1:i + 1 + w], "big"))
    raise ValueError(f"msgpack type {t:#x} not handled")


def _arr(b, i, n):
    out = []
    for _ in range(n):
        v, i = _unpack(b, i)
        out.append(v)
    return out, i


def _map(b, i, n):
    out = {}
    for _ in range(n):
        k, i = _unpack(b, i)
        v, i = _unpack(b, i)
        out[k] = v
    return out, i


def _code_objects(data):
    """the gfx950 ELF images of every offload bundle in the file"""
    at = data.find(MAGIC)
    while at >= 0:
        n = struct.unpack_from("<Q", data, at + len(MAGIC))[0]
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode(errors="replace")
            p += 24 + tlen
            if "gfx950" in triple and size:
                yield data[at + off:at + off + size]
        at = data.find(MAGIC, at + len(MAGIC))


def _elf_kernels(elf):
    if elf[:4] != b"\x7fELF" or elf[4] != 2:
        return {}
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + k * shentsize) for k in range(shnum)]
    meta, sizes = None, {}
    for (_, typ, _, _, off, size, link, _, _, entsize) in secs:
        if typ == 7:  # SHT_NOTE
            q = off
            while q + 12 <= off + size:
                namesz, descsz, ntype = struct.unpack_from("<III", elf, q)
                name = elf[q + 12:q + 12 + namesz].rstrip(b"\0")
                d0 = q + 12 + (namesz + 3) // 4 * 4
                if ntype == 32 and name == b"AMDGPU":
                    meta = _unpack(elf[d0:d0 + descsz], 0)[0]
                q = d0 + (descsz + 3) // 4 * 4
        elif typ == 2 and entsize:  # SHT_SYMTAB
            stroff = secs[link][4]
            for k in range(size // entsize):
                st_name, info, _, _, _, st_size = struct.unpack_from("<IBBHQQ", elf, off + k * entsize)
                if info & 0xF == 2:  # STT_FUNC
                    end = elf.index(b"\0", stroff + st_name)
                    sizes[elf[stroff + st_name:end].decode()] = st_size
    out = {}
    for k in (meta or {}).get("amdhsa.kernels", []):
        name = k[".name"]
        out[name] = {key: k.get("." + key) for key in
                     ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size",
                      "group_segment_fixed_size", "kernarg_segment_size")}
        out[name]["code_bytes"] = sizes.get(name)
        # the explicit arguments' places in the kernarg segment (hidden ones have no .value_kind "by_value" / pointer)
        out[name]["args"] = [[a.get(".offset"), a.get(".size")] for a in k.get(".args", [])
                             if not str(a.get(".value_kind", "")).startswith("hidden")]
    return out


def kernels(lib_path=DEFAULT_LIB):
    data = open(lib_path, "rb").read()
    out = {}
    for elf in _code_objects(data):
        out.update(_elf_kernels(elf))
    return out


def find(lib_path, *subs):
    hits = {n: v for n, v in kernels(lib_path).items() if all(s in n for s in subs)}
    if len(hits) != 1:
        raise LookupError(f"{len(hits)} kernels of {lib_path} match {subs}: {sorted(hits)}")
    return next(iter(hits.items()))


if __name__ == "__main__":
    lib = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_LIB
    subs = sys.argv[2:] or ["wf_finish_bvh", "wf_long"]
    for name, v in sorted(kernels(lib).items()):
        if any(s in name for s in subs):
            print(json.dumps({"kernel": name, **v}))
