"""Do two builds of libhierdiff_hip.so hold the same device code?

    python scratch/kernel_bytes.py A/libhierdiff_hip.so B/libhierdiff_hip.so

Takes the gfx950 code object out of each library's .hip_fatbin section (an uncompressed clang offload bundle) and hashes the bytes of
every kernel (function symbol) and every kernel descriptor (object symbol: register counts, LDS and scratch sizes).  Prints the
number of each, whether the whole code objects are byte-identical, and every symbol that is missing on one side or differs in size
or bytes.  Exit status 0: same set of symbols, each with the same size and bytes.  (readelf lists every kernel twice, in .symtab
and in .dynsym; this reads .symtab.  `__hip_cuid_<hash>`, one byte whose NAME is a hash of the source file's path, is left out: it
differs between two checkouts of the same source, and is what keeps their code objects from being byte-identical.  In a kernel
descriptor, bytes 16..23 - the distance from the descriptor to the kernel's first instruction - are left out too: they move with the
size of every kernel placed in front, so one changed kernel would report all descriptors behind it.)"""
import hashlib
import struct
import sys

BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def sections(elf):
    """{name: (type, addr, offset, size, link, entsize)} of an ELF64 little-endian image."""
    assert elf[:6] == b"\x7fELF\x02\x01", "not an ELF64 LE image"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    raw = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]
    strtab = raw[shstrndx]
    name = lambda off: elf[strtab[4] + off:elf.index(b"\0", strtab[4] + off)].decode()
    return {name(s[0]): (s[1], s[3], s[4], s[5], s[6], s[9]) for s in raw}, raw


def code_object(lib_path, target="gfx950"):
    elf = open(lib_path, "rb").read()
    secs, _ = sections(elf)
    _, _, off, size, _, _ = secs[".hip_fatbin"]
    fat = elf[off:off + size]
    assert fat[:len(BUNDLE_MAGIC)] == BUNDLE_MAGIC, "the fat binary is not an uncompressed offload bundle"
    n, = struct.unpack_from("<Q", fat, len(BUNDLE_MAGIC))
    pos = len(BUNDLE_MAGIC) + 8
    for _ in range(n):
        o, s, idlen = struct.unpack_from("<QQQ", fat, pos)
        ident = fat[pos + 24:pos + 24 + idlen].decode()
        pos += 24 + idlen
        if ident.startswith("hip") and ident.endswith(target):
            return fat[o:o + s]
    raise SystemExit(f"{lib_path}: no {target} entry in the bundle")


def functions(co):
    """{symbol: (type, size, sha256 of its bytes)} for every defined function (2) and object (1) symbol of a code object."""
    secs, raw = sections(co)
    _, _, off, size, link, entsize = secs[".symtab"]
    str_off = raw[link][4]
    out = {}
    for i in range(size // entsize):
        st_name, st_info, _, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", co, off + i * entsize)
        if st_info & 0xF not in (1, 2) or st_shndx == 0:          # STT_OBJECT / STT_FUNC, defined
            continue
        name = co[str_off + st_name:co.index(b"\0", str_off + st_name)].decode()
        if name.startswith("__hip_cuid_"):
            continue
        sec = raw[st_shndx]
        start = sec[4] + (st_value - sec[3])
        body = co[start:start + st_size]
        if name.endswith(".kd") and st_size == 64:
            body = body[:16] + body[24:]                          # kernel_code_entry_byte_offset
        out[name] = (st_info & 0xF, st_size, hashlib.sha256(body).hexdigest())
    return out


def main():
    a_path, b_path = sys.argv[1:3]
    a_co, b_co = code_object(a_path), code_object(b_path)
    a, b = functions(a_co), functions(b_co)
    count = lambda d, ty: sum(1 for v in d.values() if v[0] == ty)
    print(f"function symbols: {count(a, 2)} / {count(b, 2)}; object symbols: {count(a, 1)} / {count(b, 1)}; code objects: {len(a_co)} / {len(b_co)} bytes, "
          f"{'byte-identical' if a_co == b_co else 'not byte-identical'}")
    bad = 0
    for name in sorted(set(a) | set(b)):
        if a.get(name) != b.get(name):
            bad += 1
            print(f"DIFFERS {name}: {a.get(name)} / {b.get(name)}")
    print(f"{bad} symbols differ")
    return 1 if bad else 0


if __name__ == "__main__":
    raise SystemExit(main())
