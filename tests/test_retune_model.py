"""The retune model (tests/retune_ref.py) is a valid oracle: with no retune it reproduces liborc's orc_vfo bit for bit, and
topology.mix_offset_retune gives the sub mixers topology_from_ini derives from the new offset (mainwindow.cpp:141-225)."""
import dataclasses

import numpy as np
import pytest

from oracle import binding as ob
from sdrreceiver_amd import synth, topology as tp
import retune_ref as rr

FRAMES = 4


def _oracle_frames(topo, leaf, n_frames=FRAMES, seed=5):
    """Runs `topo` on the oracle; per frame: (input of node `leaf`, its stream, its payload)."""
    nodes, roots = ob.build_tree("port", topo)
    lcg = synth.Lcg(seed)
    out = []
    for _ in range(n_frames):
        iq = synth.lcg_frame(topo.frame, lcg)
        ob.process_roots(roots, iq)
        p = topo.vfos[leaf].parent
        x = iq.view(np.complex64) if p < 0 else nodes[p].stream()
        v = nodes[leaf]
        pay = v.usb() if topo.vfos[leaf].demod_usb else v.iq()
        out.append((x.copy(), v.stream(), pay))
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


CASES = {
    "config1_sub_d5_lpf4k": (tp.config1(), 1),
    "sub_48k_lpf10k": (tp.subset(tp.config3(8), [7])[0], 1),      # main1 (d=3, 192 k) -> d=2 -> 48 k, 10 kHz low-pass
    "leaf_div5_1920k": (tp.subset(tp.config4(3), [3])[0], 1),     # 240 k, d=0, late /5, 10 kHz low-pass
    "compress_main": (dataclasses.replace(tp.config1(), vfos=[tp.config1().vfos[0]]), 0),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_model_equals_orc_vfo_without_retune(case):
    topo, leaf = CASES[case]
    want = _oracle_frames(topo, leaf)
    got = rr.run(topo.vfos[leaf], [w[0] for w in want])
    for f, ((_, s, p), (gs, gp)) in enumerate(zip(want, got)):
        assert np.array_equal(_bits(gs), _bits(s)), f"{case} frame {f}: stream"
        assert p.size > 0 and np.array_equal(_bits(gp), _bits(p)), f"{case} frame {f}: payload"


def test_model_gain_change_equals_orc_set_gain():
    """A gain change between frames is orc_vfo_set_gain between two orc_vfo_process calls."""
    topo = tp.config1()
    nodes, roots = ob.build_tree("port", topo)
    node = rr.Node(topo.vfos[1])
    lcg = synth.Lcg(9)
    for f in range(3):
        if f == 1:
            nodes[1].setGain(0.5)
            node.set_gain(0.5)
        iq = synth.lcg_frame(topo.frame, lcg)
        ob.process_roots(roots, iq)
        node.process(nodes[0].stream())
        assert np.array_equal(node.payload(), nodes[1].usb()), f"frame {f}"


def test_model_retune_restarts_the_oscillator():
    """After a retune at frame K the mixer multiplies by a fresh oscillator's sequence: entry L-1, then 1, 2, ..."""
    d = tp.config1().vfos[1]
    node = rr.Node(d)
    x = np.ones(d.samples_per_buffer, np.complex64)
    node.process(x)
    node.retune(12345.0)
    z = rr.mix(node.tab, node.k, x)
    seq = ob.osc_sequence("port", d.fs, 12345.0, x.size)
    assert np.array_equal(_bits(z), _bits(seq))


INI_25E_LIKE = """
[General]
sample_rate=1536000
center_frequency=1545600000
zmq_address=tcp://*:6003
correct_dc_bias=1
mix_offset=0

[main_vfos]
size=2
1\\frequency=1545116000
1\\out_rate=384000
2\\frequency=1546096000
2\\out_rate=192000

[vfos]
size=3
1\\frequency=1545005146
1\\gain=5
1\\filter_bandwidth=4000
1\\data_rate=600
1\\topic=VFO01
2\\frequency=1545124261
2\\gain=5
2\\data_rate=1200
2\\topic=VFO07
3\\frequency=1546137300
3\\gain=3
3\\data_rate=10500
3\\filter_bandwidth=10000
3\\topic=VFO19
"""


def config3_ini(n_subs: int = 1024, mix_offset: int = 0) -> str:
    """An INI whose topology_from_ini is BASELINE config 3 (mains of sdr_25E; half the subs at 12 k on main 1, half at 48 k on
    main 2, every 2nd of those with the 10 kHz low-pass, gain 5 %)."""
    t = tp.config3(n_subs)
    center = t.center_frequency
    lines = ["[General]", "sample_rate=1536000", f"center_frequency={center}", f"mix_offset={mix_offset}", "",
             "[main_vfos]", "size=2"]
    mains = t.roots()
    for i, m in enumerate(mains, 1):
        v = t.vfos[m]
        lines += [f"{i}\\frequency={center - int(v.mixer_freq)}", f"{i}\\out_rate={v.out_rate_stage}"]
    subs = [i for i, v in enumerate(t.vfos) if v.parent >= 0]
    lines += ["", "[vfos]", f"size={len(subs)}"]
    for k, i in enumerate(subs, 1):
        v, m = t.vfos[i], t.vfos[t.vfos[i].parent]
        freq = center - int(m.mixer_freq) - int(v.mixer_freq) - mix_offset
        lines += [f"{k}\\frequency={freq}", f"{k}\\gain=5", f"{k}\\out_rate={v.output_rate}", f"{k}\\topic={v.topic}"]
        if v.filter_bw:
            lines.append(f"{k}\\filter_bandwidth={v.filter_bw}")
    return "\n".join(lines) + "\n"


def test_config3_ini_is_config3():
    assert tp.topology_from_ini(config3_ini(64)).vfos == tp.config3(64).vfos


@pytest.mark.parametrize("ini", ["25e", "config3"])
def test_mix_offset_retune_equals_the_ini_rule(ini):
    text = INI_25E_LIKE if ini == "25e" else config3_ini(64)
    topo = tp.topology_from_ini(text)
    for off in (1500, -2500, 37):
        ids, freqs = tp.mix_offset_retune(topo, text, off)
        want = tp.topology_from_ini(text.replace("mix_offset=0", f"mix_offset={off}"))
        assert ids == [i for i, v in enumerate(topo.vfos) if v.parent >= 0]
        assert freqs == [want.vfos[i].mixer_freq for i in ids]
        assert all(f == topo.vfos[i].mixer_freq - off for i, f in zip(ids, freqs))
        # the retuned tree is the new INI's tree
        retuned = list(topo.vfos)
        for i, f in zip(ids, freqs):
            retuned[i] = dataclasses.replace(retuned[i], mixer_freq=f)
        assert retuned == want.vfos


def test_mix_offset_retune_refuses_a_new_geometry():
    """-700 000 Hz carries VFO19 into main 1's band (test_topology.py::test_ini_rules_with_a_mix_offset): a new tree."""
    topo = tp.topology_from_ini(INI_25E_LIKE)
    with pytest.raises(ValueError, match="new tree"):
        tp.mix_offset_retune(topo, INI_25E_LIKE, -700000)
    with pytest.raises(ValueError):
        tp.mix_offset_retune(tp.config1(), INI_25E_LIKE, 100)
