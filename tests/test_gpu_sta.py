"""GPU STA numerics vs CPU fp32 reference (same graph, random delays)."""
import numpy as np
import pytest

from parallel_eda_amd.arch.archdef import get_arch
from parallel_eda_amd.io.synth import synth_netlist, spec_for_arch, SynthSpec
from parallel_eda_amd.timing.sta import STA

pytestmark = pytest.mark.gpu


def test_gpu_sta_matches_cpu():
    from parallel_eda_amd.timing.gpu_sta import GpuSTA
    arch = get_arch("tseng")
    nl = synth_netlist(SynthSpec(n_clb=300, n_in=12, n_out=12, seed=21,
                                 max_fanin=16))
    cpu_sta = STA(nl, arch)
    gpu_sta = GpuSTA(nl, arch)
    rng = np.random.default_rng(3)
    for trial in range(3):
        d = (rng.random(nl.num_conns) * 2e-9).astype(np.float32)
        cpd_c, slack_c, crit_c = cpu_sta.analyze(d)
        cpd_g, slack_g, crit_g = gpu_sta.analyze(d)
        # cpd and slack are chains of single fp32 +, -, max, min: equal
        # to the bit (tests/test_sta_exact.py has the derivation)
        assert np.float32(cpd_g) == np.float32(cpd_c)
        assert np.array_equal(slack_g, slack_c)
        # GPU clamps crit to 0.99; apply same clamp to CPU reference. The
        # kernel multiplies by 1/cpd where the CPU divides: <= 6 * 2^-24
        crit_c2 = np.minimum(crit_c, np.float32(0.99))
        assert np.abs(crit_g.astype(np.float64) - crit_c2).max() <= 6 * 2.0 ** -24


def test_gpu_sta_multi_domain_matches_cpu():
    """Multi-clock-domain GPU STA vs CPU oracle (the
    domain-pair kernels were written but dormant; hardware-validated
    2026-09-14, now a standing regression gate)."""
    from parallel_eda_amd.timing.gpu_sta import GpuSTA
    arch = get_arch("tseng")
    nl = synth_netlist(spec_for_arch(arch, fill=0.5, seed=3))
    rng = np.random.default_rng(3)
    bc = np.where(np.asarray(nl.block_is_seq) > 0,
                  rng.integers(0, 2, nl.num_blocks), -1).astype(np.int32)
    periods = np.asarray([5e-9, 8e-9], dtype=np.float32)
    for trial in range(3):
        d = rng.uniform(0.1e-9, 2e-9, nl.num_conns).astype(np.float32)
        wp_c, sl_c, cr_c = STA(nl, arch).analyze_domains(d, bc, periods)
        wp_g, sl_g, cr_g = GpuSTA(nl, arch).analyze_domains(d, bc, periods)
        # one subtraction and one IEEE division on both sides: exact
        assert np.array_equal(sl_c, sl_g)
        assert np.array_equal(np.minimum(cr_c, np.float32(0.99)), cr_g)
