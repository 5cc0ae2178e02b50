"""CPU: the four-wave form of the shipped-shape PointNet backbone (csrc/kernels_infer.h pointnet_fused_duo<128, 132, 16>) keeps two weight images
(64 + 32 registers), the hidden layer's A fragments (32) and two accumulator sets live, and it only pays if two of its workgroups share a CU:
spill-free at two waves per SIMD.  The two eight-wave kernels of the shape stay instantiated, and the option that picks the form is documented."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alignnet-3d_amd", "csrc")


def _rows():
    path = os.path.join(CSRC, "alignnet_api.remarks")
    assert os.path.exists(path), "no resource remarks next to the objects: build() writes them (csrc/Makefile)"
    return re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?VGPRs Spill: (\d+)",
                      open(path).read(), re.S)


def _hits(kernel):
    return [(n, int(v), int(sc), int(occ), int(sp)) for n, v, sc, occ, sp in _rows() if kernel in n]


def test_duo_kernel_is_spill_free_at_two_waves_per_simd():
    hit = _hits("18pointnet_fused_duoILi128ELi132ELi16EE")   # pointnet_fused_duo<128, 132, 16>
    assert len(hit) == 1, hit
    name, vgpr, scratch, occ, spill = hit[0]
    print(name, "VGPRs", vgpr, "scratch", scratch, "occupancy", occ, "spilled", spill)
    assert spill == 0 and scratch == 0 and occ >= 2, hit[0]


def test_eight_wave_kernels_of_the_shape_stay_instantiated():
    for kernel in ("14pointnet_fusedILi128ELi68ELi132ELi16EE",            # pointnet_fused<128, 68, 132, 16>
                   "21pointnet_fused_streamILi128ELi68ELi132ELi16EE"):    # pointnet_fused_stream<128, 68, 132, 16>
        assert len(_hits(kernel)) == 1, (kernel, _hits(kernel))


def test_wg_waves_option_is_documented_and_dispatched():
    hdr = open(os.path.join(ROOT, "include", "alignnet_hip.h")).read()
    assert '"infer_wg_waves"' in hdr and '"last_backbone_wg_waves"' in hdr and '"backbone_wgs_per_cu"' in hdr
    api = open(os.path.join(CSRC, "alignnet_api.hip")).read()
    for key in ("infer_wg_waves", "last_backbone_wg_waves", "backbone_wgs_per_cu"):
        assert 'k == "%s"' % key in api, key
