"""bench.py's output contract: a plain run prints ONE JSON line with the driver's keys and nothing it does not need (and
writes the last step's outputs with --dump-outputs); with --full the line of <= 8 KB also holds the roofline and cpu_baseline
objects, and the secondary records (config 5, the end-to-end legs, the accuracy gates) go to a side file written by a child
process; the multi-rank path is rehearsed in tests/test_parallel_gloo.py and here (--gpus 2 / 4 over gloo on one card)."""
import json
import os
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE_LIMIT = 8192


def _bench_module():
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    import bench
    return bench


def test_line_limit_and_compaction_on_the_round5_record():
    """(CPU) the round-5 line (22 KB: the driver's parser dropped it) through this round's layout: e2e / config5 leave the
    line, their figures stay in `summary`, the line is <= 8 KB; a line that still outgrows the limit sheds its explanatory
    strings and says so, with `summary` staying the last key."""
    bench = _bench_module()
    assert bench.LINE_LIMIT == LINE_LIMIT
    old = json.load(open(os.path.join(ROOT, 'profiles', 'r05_bench_driver_cmd.json')))
    assert len(json.dumps(old)) > 20000
    detail = {'config5': old.pop('config5'), 'e2e': old.pop('e2e'), 'complete': True, 'legs_done': [['x', 1.0]] * 19,
              'file': 'bench_detail.json', 'legs_done_n': 19}
    for g in detail['e2e'].values():                      # (round 5 wrote `resolves_bar`; this round's gate fields)
        if isinstance(g, dict) and 'map_delta_vs_fp32' in g:
            lo, hi = g['map_delta_vs_fp32']['map_delta_ci95_paired_bootstrap']
            g['map_delta_vs_fp32']['ci_inside_bar'] = bool(lo >= -0.002 and hi <= 0.002)
    summary = {'hot_path_img_s': round(old['value'], 1)}
    bench.summarise_detail(summary, detail)
    assert summary['cfg5_hot_path'][0] == round(detail['config5']['value'], 1)
    assert summary['e2e_fp32_x3'][0] == round(detail['e2e']['fp32_x3']['value'], 1) and len(summary['fp32_x2']) == 4
    assert summary['map_delta_vgg16'][4] == 0 and summary['map_delta_vgg16'][1] < -0.002     # the interval the verdict quotes
    assert summary['map_delta_x3'][4] == 1 and summary['detail'] == ['bench_detail.json', 1, 19]
    old.pop('summary')
    old['summary'] = summary
    line = bench.compact_line(old)
    assert len(line) <= LINE_LIMIT and 'dropped' not in json.loads(line)
    assert len(json.dumps(summary)) <= 1024
    fat = dict(old)
    fat.pop('summary')
    fat['cpu_baseline'] = dict(fat['cpu_baseline'], sample_detail='x' * 9000)
    fat['summary'] = summary
    d = json.loads(bench.compact_line(fat))
    assert len(json.dumps(d)) <= LINE_LIMIT and d['dropped'] == ['cpu_baseline.sample_detail'] and list(d)[-1] == 'summary'


def test_detail_child_hang_does_not_cost_the_line(tmp_path, monkeypatch):
    """(CPU) the parent's side of the child protocol with a stand-in child: one that writes two legs and then hangs is killed
    at the hard limit (its own process group), the finished legs are read back, and the parent carries on."""
    bench = _bench_module()
    fake = tmp_path / 'fake_bench.py'
    fake.write_text(
        "import json, sys, time\n"
        "path = sys.argv[sys.argv.index('--detail-child') + 1]\n"
        "json.dump({'complete': False, 'legs_done': [['config5', 1.0], ['e2e fp16', 2.0]], 'config5': {'error': 'x'},\n"
        "           'e2e': {'conv_path': 'p', 'fp16': {'value': 1234.56}}}, open(path, 'w'))\n"
        "time.sleep(600)\n")
    monkeypatch.setattr(bench, '__file__', str(fake))
    import time
    args = types.SimpleNamespace(detail_out=str(tmp_path / 'd.json'), time_budget=-20.0, steps=1, warmup=1, rounds_per_step=1,
                                 streams=1, batch=1, blind_chunks=1, nms_first_chunk=0, roofline_samples=3, gate_images=128,
                                 no_e2e=False, no_config5=False, trace=False)
    t0 = time.perf_counter()
    # (budget = max(time_budget - elapsed - 5, 1) = 1 s; hard limit = budget + 25 s: shortened here)
    monkeypatch.setattr(bench, 'HARD_LIMIT_EXTRA_S', 2.0)
    detail = bench.run_detail_child(args, t0)
    assert time.perf_counter() - t0 < 30.0
    assert detail['complete'] is False and 'killed' in str(detail['child_rc']) and detail['legs_done_n'] == 2
    summary = {}
    bench.summarise_detail(summary, detail)
    assert summary['e2e_fp16'] == [1234.6, 60] and summary['cfg5_hot_path'] == 'error' and summary['detail'][1] == 0
    assert json.load(open(args.detail_out))['child_rc'] == detail['child_rc']
    # a SIGTERM handler installed from C (rocprofv3 does) reads back as None: restoring it must not raise (round 6: this lost
    # the line of the profiled run)
    import signal
    real = signal.signal
    monkeypatch.setattr(signal, 'signal', lambda signum, h: None if callable(h) and h.__name__ == 'on_term' else real(signum, h))
    detail = bench.run_detail_child(args, time.perf_counter())
    assert detail['legs_done_n'] == 2


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_keys(tmp_path):
    # (the driver's own command line with --full, plus --no-e2e: the end-to-end detector records and their accuracy gates
    # take minutes)
    side = str(tmp_path / 'detail.json')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5',
                        '--full', '--no-e2e', '--detail-out', side], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1 and len(lines[0]) <= LINE_LIMIT
    d = json.loads(lines[0])
    assert 'e2e' not in d and 'config5' not in d          # (bulky records live in the side file)
    side_rec = json.load(open(side))
    assert d['detail']['complete'] is True and d['detail']['child_rc'] == 0 and side_rec['complete'] is True
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in d, k
    assert d['metric'] == 'images/sec' and d['unit'] == 'img/s' and d['n_gpus'] == 1 and d['steps'] == 20 and d['warmup'] == 5
    assert d['higher_is_better'] is True and d['scaling'] == 'weak' and d['vs_baseline'] is None
    assert d['dtype'] == 'f32' and d['data'] == 'synthetic' and 'workload' in d['config'] and 'model' not in d['config']
    r = d['roofline']
    assert r['bound'] == 'hbm' and r['unit'] == 'GB/s' and r['peak'] == 8000.0
    assert r['kernel_ms'] > 0 and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-9 and r['kernel_ms_samples'] >= 10
    assert r['B_min'] <= r['algorithmic_bytes'] <= r['B_taps'] and r['bytes_output'] < r['B_min']
    assert abs(r['achieved'] - r['algorithmic_bytes'] / (r['kernel_ms'] * 1e-3) / 1e9) < 1e-6 * r['achieved']
    if r['traffic'] is not None:
        assert abs(r['hbm_frac_measured'] - r['traffic'] / (r['kernel_ms'] * 1e-3) / 8e12) < 1e-9
    assert 'k_roi_pool' in r['rocprof_kernel_name']
    cal = r['calibration']            # the same bytes moved by a kernel that does nothing else, same protocol
    assert cal['samples'] >= 5 and cal['ms'] > 0 and cal['bytes_written'] <= r['bytes_output']
    assert abs(cal['roi_kernel_vs_calibration'] - cal['ms'] / r['kernel_ms']) < 1e-9
    assert 0.3 < cal['roi_kernel_vs_calibration'] < 1.5
    c = d['cpu_baseline']
    assert c['kind'] == 'port' and c['unit'] == 'img/s' and c['value'] > 0 and c['cores'] >= 1 and 'sample' in c
    assert abs(c['map_delta']['delta']) <= 0.002
    # both thread modes of BASELINE.md section 3, a bounded sample of each
    assert c['value_1thread'] > 0 and c['value_threads'] > 0 and c['samples'] >= 8 and c['samples_1thread'] >= 4
    assert abs(c['value'] - max(c['value_1thread'], c['value_threads'])) < 1e-9 and c['cores'] in (1, c['threads'])   # the faster leg
    # the other RPN score distribution (trained-like clusters) in the same line, its own timed region; the bench widens
    # its sync-free NMS plan by itself instead of aborting
    assert d['value_clustered'] > 0 and d['ms_per_step_clustered'] > 0
    sd = d['config']['second_distribution']
    assert sd['rpn_scores'] == 'clustered' and sd['proposals_kept'] == 1000
    assert abs(sd['ms_per_step'] * sd['value'] / (1000.0 * d['config']['images_per_step_per_gpu']) - 1.0) < 1e-6
    # a step = images_per_step_per_gpu images on every GPU; the driver's 20 steps time at least half a second
    ips = d['config']['images_per_step_per_gpu']
    assert ips == 48 * d['config']['streams_per_gpu'] * d['config']['images_per_launch']
    assert d['value'] > 0 and abs(d['ms_per_step'] * d['value'] / (1000.0 * ips * d['n_gpus']) - 1.0) < 1e-6
    assert d['config']['timed_region_s'] >= 0.3 and d['config']['timed_images'] == 20 * ips
    # BASELINE configs[4] as a measured record: 1333 x 1333, 446 118 anchors, 81 classes, caps 100 / 300, float16 maps
    c5 = side_rec['config5']
    assert 'error' not in c5, c5
    assert c5['anchors'] == 446118 and c5['num_classes'] == 81 and c5['max_per_class'] == 100 and c5['max_per_image'] == 300
    assert c5['value'] > 0 and c5['dtype'] == 'f16' and c5['proposals_kept'] == 1000 and 0 < c5['detections_image0'] <= 300
    r5 = c5['roofline']
    assert r5['kernel_ms'] > 0 and '__half' in r5['rocprof_kernel_name'] and r5['B_min'] <= r5['algorithmic_bytes']
    # what a multi-GPU run needs to check itself (one rank here: no exchange in the loop)
    mr = d['multi_rank']
    assert mr['rccl_world'] == 1 and mr['ranks_timed'] == 1 and mr['allgathers_in_timed_region'] == 0
    assert abs(mr['per_rank_img_s_min'] - d['value']) < 1e-6 * d['value'] and mr['per_rank_spread'] == 0
    # the compact LAST key: every headline figure inside the tail of the line the driver keeps
    assert list(d.keys())[-1] == 'summary'
    sm = d['summary']
    assert len(json.dumps(sm)) <= 1024
    assert sm['hot_path_img_s'] == round(d['value'], 1) and sm['cfg5_hot_path'][0] == round(c5['value'], 1)
    assert sm['ranks'][0] == 1 and sm['cpu_port_img_s'][0] == round(c['value'], 1) and sm['detail'][1] == 1


@pytest.mark.gpu
def test_bench_e2e_summary_keys(tmp_path):
    """the end-to-end part on a reduced gate (256 scenes): batch-1 (HIP graph) / 4 / 8 legs, all three families, their
    accuracy gates -- in the side file -- and the summary of the line that carries their figures"""
    side = str(tmp_path / 'detail.json')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '4', '--warmup', '1',
                        '--full', '--no-cpu-baseline', '--no-config5', '--no-second-distribution', '--gate-images', '256',
                        '--time-budget', '900', '--detail-out', side], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1200)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1 and len(lines[0]) <= LINE_LIMIT
    d = json.loads(lines[0])
    assert 'e2e' not in d and d['detail']['complete'] is True
    e = json.load(open(side))['e2e']
    for leg in ('fp16', 'fp16_b1', 'fp16_b4', 'fp16_b8', 'fp32', 'fp32_x3', 'fp32_x2', 'fp16_resnet50_c4', 'fp16_vgg16_600x800'):
        assert 'error' not in e[leg], (leg, e[leg])
        assert e[leg]['value'] > 0 and e[leg]['nms_done'] == 1
    assert e['fp16_b1']['batch'] == 1 and e['fp16_b1']['value_hip_graph'] > e['fp16_b1']['value'] * 0.9
    for leg, fam in (('fp16', 'fpn'), ('fp16_resnet50_c4', 'c4'), ('fp16_vgg16_600x800', 'vgg16')):
        g = e[leg]['map_delta_vs_fp32']
        assert g['family'] == fam and g['images'] >= 256 and abs(g['map_delta']) < 0.02
        lo, hi = g['map_delta_ci95_paired_bootstrap']
        assert g['ci_inside_bar'] == (lo >= -0.002 and hi <= 0.002) and 'resolves_bar' not in g and 'ci_half_width_within_bar' in g
    # the float32 split-precision mode: faster than the exact-float32 mode, and the same detector up to float32 rounding
    gx = e['fp32_x3']['map_delta_vs_fp32']
    assert e['fp32_x3']['value'] > 1.2 * e['fp32']['value'] and abs(gx['map_delta']) < 1e-3
    assert gx['rpn_kept_index_agreement_mean'] > 0.995 and gx['p99_abs_dscore'] < 1e-3
    # the two-limb float16 form of the same mode: faster again, the same detector up to float32 rounding
    g2 = e['fp32_x2']['map_delta_vs_fp32']
    assert e['fp32_x2']['value'] > 1.1 * e['fp32_x3']['value'] and abs(g2['map_delta']) < 1e-3
    assert g2['rpn_kept_index_agreement_mean'] > 0.995 and g2['p99_abs_dscore'] < 1e-3
    sm = d['summary']
    assert list(d.keys())[-1] == 'summary' and len(json.dumps(sm)) <= 1024
    assert sm['fp32_x2'][0] == round(e['fp32_x2']['value'], 1) and len(sm['fp32_x2']) == 4
    assert sm['e2e_fp32_x3'][0] == round(e['fp32_x3']['value'], 1) and len(sm['map_delta_x3']) == 5
    assert sm['e2e_fp16_b1_graph'] == round(e['fp16_b1']['value_hip_graph'], 1) and sm['e2e_fp16'][0] == round(e['fp16']['value'], 1)
    assert sm['map_delta_fpn'][3] == 256 and len(sm['map_delta_c4']) == 5 and len(sm['map_delta_vgg16']) == 5
    assert sm['map_delta_fpn'][4] == int(e['fp16']['map_delta_vs_fp32']['ci_inside_bar'])


def _one_line(cmd, timeout=900):
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.strip().startswith('{')]
    assert len(lines) == 1, p.stdout.decode()[-2000:]
    assert len(lines[0]) <= LINE_LIMIT
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_gpus_2_starts_its_own_ranks():
    """VERDICT r4 missing #1: the driver's plain `python bench.py --gpus N` (no launcher environment) starts its N ranks itself
    as fresh child processes and relays rank 0's line.  On a 1-GPU box the ranks share the card over gloo (--backend gloo); the
    record validates itself: ranks seen by the backend, all-gathers issued == expected, per-rank rates."""
    d = _one_line([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1', '--backend', 'gloo',
                   '--no-second-distribution'])
    assert d['n_gpus'] == 2 and d['scaling'] == 'weak' and d['value'] > 0
    mr = d['multi_rank']
    assert mr['world_size_env'] == 2 and mr['rccl_world'] == 2 and mr['ranks_timed'] == 2 and mr['backend'] == 'gloo'
    assert mr['allgathers_in_timed_region'] == mr['allgathers_expected'] == 2 * 48 * d['config']['streams_per_gpu']
    ips = d['config']['images_per_step_per_gpu']
    assert d['config']['global_batch'] == 2 * ips and d['config']['timed_images'] == 2 * 2 * ips
    assert abs(d['ms_per_step'] * d['value'] / (1000.0 * ips * 2) - 1.0) < 1e-6
    assert d['config']['nms_reruns'] == 0 and d['summary']['ranks'][0] == 2
    # the torchrun form of the driver's multi-GPU command keeps working (one rank here, the RCCL collective forced)
    d = _one_line([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr', '127.0.0.1',
                   '--master-port', '29641', os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1',
                   '--force-collective', '--no-second-distribution', '--no-e2e', '--no-cpu-baseline', '--no-config5'])
    mr = d['multi_rank']
    assert mr['backend'] == 'nccl' and mr['rccl_world'] == 1
    assert mr['allgathers_in_timed_region'] == mr['allgathers_expected'] > 0


@pytest.mark.gpu
def test_bench_gpus_4_at_the_drivers_step_counts_prints_one_small_line():
    """config 4 launch-ready -- `python bench.py --gpus 4 --steps 20 --warmup 5` (the driver's step counts; the
    four ranks share this box's card over gloo): one line of <= 8 KB, rc 0, every rank timed, every stream group's all-gather
    issued inside the timed region."""
    d = _one_line([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '4', '--steps', '20', '--warmup', '5', '--backend', 'gloo'],
                  timeout=1200)
    assert d['n_gpus'] == 4 and d['scaling'] == 'weak' and d['steps'] == 20 and d['warmup'] == 5 and d['value'] > 0
    mr = d['multi_rank']
    assert mr['ranks_timed'] == 4 and mr['rccl_world'] == 4 and mr['world_size_env'] == 4
    assert mr['allgathers_in_timed_region'] == mr['allgathers_expected'] == 20 * 48 * d['config']['streams_per_gpu']
    assert d['config']['global_batch'] == 4 * d['config']['images_per_step_per_gpu'] and d['config']['nms_reruns'] == 0
    assert 'cpu_baseline' not in d and 'detail' not in d and list(d)[-1] == 'summary' and d['summary']['ranks'][0] == 4


def _fake_slots(n, K, M, P, C, seed=0):
    import numpy as np
    import torch
    g = torch.Generator().manual_seed(seed)
    return [types.SimpleNamespace(
        det_boxes=torch.rand((M, 4), generator=g), det_labels=torch.randint(0, 21, (M,), generator=g, dtype=torch.int32),
        det_scores=torch.rand(M, generator=g), det_count=torch.tensor([M - s], dtype=torch.int32),
        sorted_rois=torch.rand((K, 4), generator=g), roi_count=torch.tensor([K], dtype=torch.int32),
        roi_features=torch.randn((K, P, P, C), generator=g).to(torch.float16 if s % 2 else torch.float32))
        for s in range(n)], torch.from_numpy(np.arange(n * (M * 6 + 1), dtype=np.float32).reshape(n, M * 6 + 1))


def test_dump_outputs_writes_the_last_steps_arrays_within_the_limit(tmp_path, monkeypatch):
    """(CPU) --dump-outputs: every array of the path's outputs as <name>.npy in float32 / float64, the pooled features as
    per-RoI float64 sums plus the full features of a fixed, seeded choice of RoIs (the same rows in every run), < 64 MB"""
    import numpy as np
    bench = _bench_module()
    slots, records = _fake_slots(3, 100, 5, 7, 16)
    shapes = bench.dump_outputs(slots, records, str(tmp_path / 'a'))
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == sorted(k + '.npy' for k in shapes) and len(files) == 10
    d = {k: np.load(str(tmp_path / 'a' / (k + '.npy'))) for k in shapes}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert d['det_boxes'].shape == (3, 5, 4) and d['det_count'].tolist() == [5, 4, 3] and d['records'].shape == (3, 31)
    np.testing.assert_array_equal(d['det_labels'][1], slots[1].det_labels.numpy())
    np.testing.assert_array_equal(d['proposals'][2], slots[2].sorted_rois.numpy())
    rows = d['roi_features_sample_rows'].astype(np.int64)
    assert len(rows) == 32 and np.all(np.diff(rows) > 0)
    for s in range(3):
        f = slots[s].roi_features.float().numpy()
        np.testing.assert_array_equal(d['roi_features_sample'][s], f[rows])
        np.testing.assert_allclose(d['roi_feature_sums'][s], f.reshape(100, -1).astype(np.float64).sum(1), rtol=1e-12, atol=1e-9)
    bench.dump_outputs(slots, records, str(tmp_path / 'b'))            # same rows, same bytes
    for k in shapes:
        assert open(str(tmp_path / 'a' / (k + '.npy')), 'rb').read() == open(str(tmp_path / 'b' / (k + '.npy')), 'rb').read()
    # the default arrangement (24 images in flight, 1000 RoIs of 7 x 7 x 256) stays under the limit; fewer sampled RoIs when
    # more images are in flight; and a dump that would still outgrow the limit is an error, not a silent truncation
    n, row = 24, 7 * 7 * 256 * 4
    assert 24 * (min(32, bench.DUMP_FEATURE_BYTES // (n * row)) * row + 1000 * (16 + 8) + 50 * 24 + 301 * 4 + 16) < bench.DUMP_LIMIT
    monkeypatch.setattr(bench, 'DUMP_FEATURE_BYTES', 3 * 8 * 7 * 7 * 16 * 4)
    assert bench.dump_outputs(slots, records, str(tmp_path / 'c'))['roi_features_sample'][1] == 8
    monkeypatch.setattr(bench, 'DUMP_LIMIT', 1000)
    with pytest.raises(SystemExit):
        bench.dump_outputs(slots, records, str(tmp_path / 'd'))


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_step(tmp_path):
    """The plain command (no --full) times exactly --steps steps, prints the driver's keys and nothing that needs runs of its
    own, and --dump-outputs writes what the timed path computed: image 0 of the last step is the oracle's answer on the
    seeded inputs (proposals in level order, detections, pooled features of the sampled RoIs)."""
    import numpy as np
    from oracle import c_oracle as co
    from tf_eager_object_detection_amd.pipeline import synthetic_fpn_inputs
    out = tmp_path / 'dump'
    d = _one_line([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                   '--dump-outputs', str(out)], timeout=600)
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'n_gpus', 'steps', 'warmup', 'config'):
        assert k in d, k
    for k in ('roofline', 'cpu_baseline', 'detail', 'value_clustered'):
        assert k not in d, k
    assert d['metric'] == 'images/sec' and d['unit'] == 'img/s' and d['higher_is_better'] is True and d['dtype'] == 'f32'
    ips = d['config']['images_per_step_per_gpu']
    assert d['steps'] == 3 and d['config']['timed_images'] == 3 * ips
    assert abs(d['ms_per_step'] * 3 - d['config']['timed_region_s'] * 1e3) < 1e-6 * d['ms_per_step']
    assert abs(d['ms_per_step'] * d['value'] / (1000.0 * ips) - 1.0) < 1e-6 and list(d)[-1] == 'summary'
    a = {f[:-4]: np.load(str(out / f)) for f in os.listdir(out)}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    n = d['config']['images_in_flight_per_gpu']
    assert a['det_count'].shape == (n,) and a['proposal_count'].tolist() == [1000] * n
    rows = a['roi_features_sample_rows'].astype(np.int64)
    np.testing.assert_allclose(a['roi_feature_sums'][:, rows],
                               a['roi_features_sample'].reshape(n, len(rows), -1).astype(np.float64).sum(2), rtol=1e-9, atol=1e-6)
    # image 0 = the seeded inputs the bench gives slot 0, through the oracle
    shape = (800, 1333)
    host, _ = synthetic_fpn_inputs(shape, 21, 1000, 256, seed=1234, device='cpu')
    rois, _ = co.region_proposal(host['rpn_deltas'], co.fpn_anchors(shape), co.rpn_fg_fpn(host['rpn_logits']), shape, 1000, 0.7)
    lv, perm, _ = co.assign_levels(rois)
    srois, slv = rois[perm], lv[perm]
    np.testing.assert_array_equal(a['proposals'][0], srois)
    for r in rows:
        want = co.roi_pool(host['feats'][int(slv[r]) - 2], srois[r:r + 1], image_shape=shape, pool=7)[0]
        np.testing.assert_array_equal(a['roi_features_sample'][0, list(rows).index(r)], want)
    wb, wl, ws = co.post_ops(host['cls_scores'], host['cls_deltas'], srois, shape, [0, 0, 0, 0], [.1, .1, .2, .2],
                             50, 50, 0.3, 0.0, 16, 21)
    m = int(a['det_count'][0])
    assert m == len(ws)
    np.testing.assert_array_equal(a['det_labels'][0, :m], wl)
    np.testing.assert_array_equal(a['det_scores'][0, :m], ws)
    assert m == 0 or np.max(np.abs(a['det_boxes'][0, :m] - wb)) <= 1e-4 * max(1.0, float(np.abs(wb).max()))
