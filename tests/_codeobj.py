"""Read per-kernel resource usage (VGPRs, spills, LDS) out of the gfx950 code objects embedded in a HIP
shared library: the clang offload bundles in .hip_fatbin, then the AMDGPU metadata note (msgpack) of each ELF."""
import struct

import msgpack

_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(path, arch="gfx950"):
    blob = open(path, "rb").read()
    pos = 0
    while True:
        i = blob.find(_MAGIC, pos)
        if i < 0:
            return
        n, = struct.unpack_from("<Q", blob, i + 24)
        o = i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, o)
            triple = blob[o + 24:o + 24 + tl].decode()
            o += 24 + tl
            if arch in triple and size:
                yield blob[i + off:i + off + size]
        pos = i + 24


def kernels(elf):
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    for k in range(shnum):
        sh = elf[shoff + k * shentsize: shoff + (k + 1) * shentsize]
        if struct.unpack_from("<I", sh, 4)[0] != 7:  # SHT_NOTE
            continue
        off, size = struct.unpack_from("<QQ", sh, 0x18)
        p = off
        while p < off + size:
            namesz, descsz, ntype = struct.unpack_from("<III", elf, p)
            name = elf[p + 12:p + 12 + namesz]
            d0 = p + 12 + ((namesz + 3) & ~3)
            desc = elf[d0:d0 + descsz]
            p = d0 + ((descsz + 3) & ~3)
            if ntype == 32 and name.startswith(b"AMDGPU"):  # NT_AMDGPU_METADATA
                for kern in msgpack.unpackb(desc, raw=False, strict_map_key=False).get("amdhsa.kernels", []):
                    yield kern


def kernel_table(path):
    """{mangled kernel name: metadata dict} for every gfx950 kernel in the library"""
    return {k[".name"]: k for co in code_objects(path) for k in kernels(co)}


# The localised kernels' family as their template argument: GcFamily (efa_gcsweep.hip) for the two sweep forms, ImpactFactor
# (efa_impact.hip) for the impact kernel, which has no adaptive form
_GC_FAMILY = {"plain": 0, "adapt": 1, "vloc": 2, "slab": 3}
_IMPACT_FACTOR = {"plain": 0, "vloc": 1, "slab": 2}


def gc_kernel_fragment(form, family, elem, *args):
    """The piece of a mangled name that picks one instantiation of a localised kernel (or, with fewer args, those that begin so):
      form "quad":   k_sweep_gc<FAM, NC, VEC, FUSED, RPL>          args = NC, VEC, FUSED, RPL   (elem "f64" only)
      form "lane":   k_sweep_gc_lane<FAM, E, MP, FUSED>            args = MP, FUSED
      form "impact": k_sweep_gc_lane_impact<MP, FAC, WIDE>         args = MP, WIDE              (elem "f64" only)
    family is "plain", "adapt", "vloc" or "slab"; elem "f64" or "f32", the rows' element type; bools are given as bools or 0 / 1
    in the places listed above.  With every arg given the fragment ends with the template list's closing E."""
    def lit(v, boolean):
        return "Lb%dE" % int(v) if boolean else "Li%dE" % int(v)

    assert elem in ("f64", "f32") and (form == "lane" or elem == "f64"), (form, elem)
    if form == "quad":
        name, full = "k_sweep_gcI", 4
        parts = [lit(_GC_FAMILY[family], False)] + [lit(v, i in (1, 2)) for i, v in enumerate(args)]
    elif form == "lane":
        name, full = "k_sweep_gc_laneI", 2
        parts = [lit(_GC_FAMILY[family], False), "d" if elem == "f64" else "f"] + [lit(v, i == 1) for i, v in enumerate(args)]
    else:
        assert form == "impact" and len(args) >= 1, (form, args)
        name, full = "k_sweep_gc_lane_impactI", 2
        parts = [lit(args[0], False), lit(_IMPACT_FACTOR[family], False)] + [lit(v, True) for v in args[1:]]
    assert len(args) <= full, (form, args)
    return name + "".join(parts) + ("E" if len(args) == full else "")


def vgpr_step(vgprs):
    """The occupancy step of a kernel: with 512 VGPRs per SIMD lane, the smallest of 128 / 168 / 256 / 512 (four, three, two
    waves per SIMD, one) that holds its registers."""
    return next(s for s in (128, 168, 256, 512) if vgprs <= s)


def assert_no_worse_than(k, before_vgprs, before_clean=True):
    """Kernel k against what the same instantiation had before a change to its source (before_vgprs its .vgpr_count,
    before_clean: it had no scratch and no VGPR spill): it stays clean, and it does not fall to a lower occupancy step."""
    if before_clean:
        assert k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0, (k[".name"], k)
    assert vgpr_step(k[".vgpr_count"]) <= vgpr_step(before_vgprs), (k[".name"], k[".vgpr_count"], before_vgprs)
