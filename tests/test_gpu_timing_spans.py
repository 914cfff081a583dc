"""GPU: when a runtime's timing spans start afresh. With the option timing_accumulate the spans of successive render calls add up
until sar_runtime_last_timing reads them; without it every render call starts with none. One launch per render call here, so one
iterate span each (sar_runtime_debug_spans, the hooks build)."""
import pytest

pytestmark = pytest.mark.gpu


def test_spans_restart_per_render_or_per_reading(sar, gpu):
    jobs, n, w, h = 256, 64, 64, 48
    cfg = sar.Config.poisson_saturne(iterations=jobs * n, width=w, height=h, jobs_total=jobs, seed=5)
    st = sar.start_points(5, 0, jobs)
    rt = sar.Runtime(cfg)
    rt.enable_timing(True)

    rt.set_option("timing_accumulate", 1)
    sar.render_jobs(cfg, rt, st)
    sar.render_jobs(cfg, rt, st)
    spans = rt.debug_spans(0)
    assert len(spans) == 2 and all(ms >= 0. for ms in spans), spans
    timing = rt.last_timing()
    assert timing.iterate_launches == 2
    assert rt.debug_spans(0) == []
    sar.render_jobs(cfg, rt, st)
    assert len(rt.debug_spans(0)) == 1

    rt.set_option("timing_accumulate", 0)   # (the option itself starts them afresh)
    assert rt.debug_spans(0) == []
    for _ in range(2):
        sar.render_jobs(cfg, rt, st)
        assert len(rt.debug_spans(0)) == 1
        assert rt.last_timing().iterate_launches == 1
        assert len(rt.debug_spans(0)) == 1   # without the option, reading clears nothing
    rt.close()
