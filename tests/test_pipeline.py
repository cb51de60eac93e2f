"""Local pipeline engine: definitions, graph paths, name mapping, stream events, parameters.

The files under ``tests/golden/definitions`` are this project's own definitions written the way
definition files of the reference kind are (``"#"`` comment keys, ``aiko_services.*`` module
names, ``class_name`` reuse, an inspector writing a file, a ``data_sources`` text pipeline);
they are loaded from disk as golden inputs, next to the inline definitions below.
"""
import json
import os
import queue
import time
from pathlib import Path

import pytest

from aiko_services_amd.pipeline.definition import (DefinitionError, parse_pipeline_definition,
                                                   parse_pipeline_definition_dict)
from aiko_services_amd.runtime import event

GOLDEN = Path(__file__).resolve().parent / "golden" / "definitions"


@pytest.fixture(scope="module")
def aiko_process():
    import aiko_services_amd as aiko
    from aiko_services_amd.message import Loopback, LoopbackBus
    if not aiko.process.initialized:
        aiko.process.run_in_thread(loop_when_no_handlers=True, message=Loopback(bus=LoopbackBus()))
    deadline = time.time() + 5
    while not event.is_running() and time.time() < deadline:
        time.sleep(0.01)
    return aiko


def _create(definition, name=None, stream_id="1", parameters=None, graph_path=None, frame_data=None,
            pathname="<inline>"):
    from aiko_services_amd.pipeline.engine import PipelineImpl
    q = queue.Queue()
    if isinstance(definition, dict):
        definition = parse_pipeline_definition_dict(definition)

    def build():
        return PipelineImpl.create_pipeline(pathname, definition, name, graph_path, stream_id,
                                            list((parameters or {}).items()), 0, frame_data, 60,
                                            queue_response=q)
    return event.call_on_loop(build), q


def _elem(name, inputs, outputs, cls=None, params=None):
    e = {"name": name, "input": [{"name": n, "type": "int"} for n in inputs],
         "output": [{"name": n, "type": "int"} for n in outputs],
         "deploy": {"local": {"module": "aiko_services_amd.examples.pipeline.elements"}}}
    if cls:
        e["deploy"]["local"]["class_name"] = cls
    if params:
        e["parameters"] = params
    return e


DIAMOND = {
    "version": 0, "name": "p_diamond", "runtime": "python",
    "graph": ["(PE_1 (PE_2 PE_4) (PE_3 PE_4) PE_Metrics)"],
    "parameters": {"p_0": None, "p_1": True, "p_2": 0, "p_3": "test"},
    "elements": [_elem("PE_1", ["b"], ["c"], params={"pe_1_inc": 1}), _elem("PE_2", ["c"], ["d"]),
                 _elem("PE_3", ["c"], ["e"]), _elem("PE_4", ["d", "e"], ["f"]),
                 _elem("PE_Metrics", [], ["f"])],
}


def test_definition_validation_errors():
    bad = dict(DIAMOND, version=1)
    with pytest.raises(DefinitionError):
        parse_pipeline_definition_dict(bad)
    bad = dict(DIAMOND, runtime="go")
    with pytest.raises(DefinitionError):
        parse_pipeline_definition_dict(bad)
    bad = json.loads(json.dumps(DIAMOND))
    bad["elements"][0]["deploy"] = {"local": {"module": "m"}, "remote": {"module": "m", "service_filter": {}}}
    with pytest.raises(DefinitionError):
        parse_pipeline_definition_dict(bad)
    bad = json.loads(json.dumps(DIAMOND))
    del bad["graph"]
    with pytest.raises(DefinitionError):
        parse_pipeline_definition_dict(bad)
    d = parse_pipeline_definition_dict(DIAMOND)
    assert d.elements[0].deploy.class_name == "PE_1"


def test_diamond_pipeline_frames(aiko_process):
    pipeline, q = _create(DIAMOND)
    for i in range(5):
        pipeline.create_frame({"stream_id": "1", "frame_id": i}, {"b": i})
    outs = [q.get(timeout=5) for _ in range(5)]
    for i, (info, data) in enumerate(outs):
        assert info["frame_id"] == i and info["state"] == 0
        # PE_1: c=b+1; PE_2: d=c+1; PE_3: e=c+1; PE_4: f=d+e
        assert data["f"] == 2 * (i + 2)
    frame_metrics_ok = pipeline.frames_completed >= 5
    assert frame_metrics_ok


def test_name_mapping_and_graph_path(aiko_process):
    d = {
        "version": 0, "name": "p_map", "runtime": "python",
        "graph": ["(PE_0 (PE_1 PE_3) (PE_2 PE_3))", "(PE_IN PE_TEXT PE_OUT)"],
        "elements": [_elem("PE_0", ["a"], ["b"]), _elem("PE_1", ["b"], ["c"]),
                     _elem("PE_2", ["c"], ["d"], cls="PE_2"), _elem("PE_3", ["c"], ["e"], cls="PE_3"),
                     {"name": "PE_IN", "input": [{"name": "in_a", "type": "str"}],
                      "output": [{"name": "text_b", "type": "str"}],
                      "deploy": {"local": {"module": "aiko_services_amd.examples.pipeline.elements"}}},
                     {"name": "PE_TEXT", "input": [{"name": "text_b", "type": "str"}],
                      "output": [{"name": "text_b", "type": "str"}],
                      "deploy": {"local": {"module": "aiko_services_amd.examples.pipeline.elements"}}},
                     {"name": "PE_OUT", "input": [{"name": "text_b", "type": "str"}],
                      "output": [{"name": "out_c", "type": "str"}],
                      "deploy": {"local": {"module": "aiko_services_amd.examples.pipeline.elements"}}}],
    }
    pipeline, q = _create(d, graph_path="PE_IN", stream_id="s1")
    pipeline.create_frame({"stream_id": "s1", "frame_id": 0}, {"in_a": "x"})
    info, data = q.get(timeout=5)
    assert data["out_c"] == "x:in:text:out"


def test_input_mapping_properties(aiko_process):
    # "(PE_0 (PE_1 PE_4 (c: d)) ...": PE_1 outputs c, PE_4 expects d and e
    d = {
        "version": 0, "name": "p_props", "runtime": "python",
        "graph": ["(PE_1 (PE_2 PE_4) (PE_3 PE_4 (e: e)))"],
        "elements": [_elem("PE_1", ["b"], ["c"]), _elem("PE_2", ["c"], ["d"]), _elem("PE_3", ["c"], ["e"]),
                     _elem("PE_4", ["d", "e"], ["f"])],
    }
    pipeline, q = _create(d, stream_id="m1")
    pipeline.create_frame({"stream_id": "m1", "frame_id": 0}, {"b": 1})
    info, data = q.get(timeout=5)
    assert data["f"] == 3 + 3


def test_drop_frame_stop_and_error(aiko_process):
    from aiko_services_amd.pipeline.stream import StreamState
    d = {
        "version": 0, "name": "p_text_sample", "runtime": "python",
        "graph": ["(TextTransform TextSample TextOutput)"],
        "elements": [
            {"name": "TextTransform", "parameters": {"transform": "uppercase"},
             "input": [{"name": "texts", "type": "[str]"}], "output": [{"name": "texts", "type": "[str]"}],
             "deploy": {"local": {"module": "aiko_services_amd.elements.media.text_io"}}},
            {"name": "TextSample", "parameters": {"sample_rate": 2},
             "input": [{"name": "texts", "type": "[str]"}], "output": [{"name": "texts", "type": "[str]"}],
             "deploy": {"local": {"module": "aiko_services_amd.elements.media.text_io"}}},
            {"name": "TextOutput", "input": [{"name": "texts", "type": "[str]"}],
             "output": [{"name": "texts", "type": "[str]"}],
             "deploy": {"local": {"module": "aiko_services_amd.elements.media.text_io"}}}],
    }
    pipeline, q = _create(d, stream_id="t1")
    for i in range(4):
        pipeline.create_frame({"stream_id": "t1", "frame_id": i}, {"texts": [f"hello {i}"]})
    outs = [q.get(timeout=5) for _ in range(4)]
    states = [info["state"] for info, _ in outs]
    assert states == [StreamState.RUN, StreamState.DROP_FRAME, StreamState.RUN, StreamState.DROP_FRAME]
    assert outs[0][1]["texts"] == ["HELLO 0"]
    # unknown transform -> ERROR -> stream destroyed immediately
    pipeline2, q2 = _create(json.loads(json.dumps(d).replace('"uppercase"', '"bogus"')), stream_id="t2")
    pipeline2.create_frame({"stream_id": "t2", "frame_id": 0}, {"texts": ["x"]})
    info, data = q2.get(timeout=5)
    assert info["state"] == StreamState.ERROR
    deadline = time.time() + 2
    while "t2" in pipeline2.stream_leases and time.time() < deadline:
        time.sleep(0.01)
    assert "t2" not in pipeline2.stream_leases


def test_text_files_data_source_target(aiko_process, tmp_path):
    src = tmp_path / "in"
    src.mkdir()
    for i in range(3):
        (src / f"in_{i:02d}.txt").write_text(f"text number {i}")
    out = tmp_path / "out"
    out.mkdir()
    d = {
        "version": 0, "name": "p_text_files", "runtime": "python",
        "graph": ["(TextReadFile TextTransform TextWriteFile)"],
        "elements": [
            {"name": "TextReadFile", "parameters": {"data_sources": f"(file://{src}/in_{{}}.txt)",
                                                    "data_batch_size": 1},
             "input": [{"name": "paths", "type": "[Path]"}], "output": [{"name": "texts", "type": "[str]"}],
             "deploy": {"local": {"module": "aiko_services_amd.elements.media.text_io"}}},
            {"name": "TextTransform", "parameters": {"transform": "titlecase"},
             "input": [{"name": "texts", "type": "[str]"}], "output": [{"name": "texts", "type": "[str]"}],
             "deploy": {"local": {"module": "aiko_services_amd.elements.media.text_io"}}},
            {"name": "TextWriteFile", "parameters": {"data_targets": f"file://{out}/out_{{:02d}}.txt"},
             "input": [{"name": "texts", "type": "[str]"}], "output": [],
             "deploy": {"local": {"module": "aiko_services_amd.elements.media.text_io"}}}],
    }
    pipeline, q = _create(d, stream_id="f1")
    outs = [q.get(timeout=10) for _ in range(3)]
    assert len(outs) == 3
    texts = sorted(p.read_text() for p in out.glob("out_*.txt"))
    assert texts == ["Text Number 0", "Text Number 1", "Text Number 2"]
    deadline = time.time() + 5   # STOP after the last frame -> graceful destroy
    while "f1" in pipeline.stream_leases and time.time() < deadline:
        time.sleep(0.05)
    assert "f1" not in pipeline.stream_leases


def test_video_files_avi_read_write(aiko_process, tmp_path):
    """VideoReadFile -> VideoWriteFile through the in-repo AVI codec (no OpenCV): a raw-DIB
    AVI is read frame by frame and written back bit-exact as a raw AVI."""
    import numpy as np
    from aiko_services_amd.elements.media import avi as A
    M = "aiko_services_amd.elements.media.video_io"
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, (18, 26, 3), dtype=np.uint8) for _ in range(4)]
    src = tmp_path / "in.avi"
    A.write_avi(src, frames, fps=10, codec="raw")
    out = tmp_path / "out.avi"
    d = {
        "version": 0, "name": "p_video_files", "runtime": "python",
        "graph": ["(VideoReadFile VideoWriteFile)"],
        "elements": [
            {"name": "VideoReadFile", "parameters": {"data_sources": f"(file://{src})"},
             "input": [{"name": "images", "type": "[image]"}], "output": [{"name": "images", "type": "[image]"}],
             "deploy": {"local": {"module": M}}},
            {"name": "VideoWriteFile", "parameters": {"data_targets": f"file://{out}", "codec": "raw", "rate": 10},
             "input": [{"name": "images", "type": "[image]"}], "output": [],
             "deploy": {"local": {"module": M}}}],
    }
    pipeline, q = _create(d, stream_id="v1")
    assert len([q.get(timeout=10) for _ in range(4)]) == 4
    deadline = time.time() + 5                      # STOP at end of file -> stop_stream closes the writer
    while "v1" in pipeline.stream_leases and time.time() < deadline:
        time.sleep(0.05)
    back = A.read_avi(out)
    assert back.shape == (4, 18, 26, 3) and all(np.array_equal(a, b) for a, b in zip(frames, back))


def test_get_parameter_precedence(aiko_process):
    from aiko_services_amd.pipeline.engine import PipelineElementImpl
    pipeline, q = _create(DIAMOND, stream_id="pp", parameters={"PE_1.pe_1_inc": 7, "p_3": "stream"})
    pe_1 = pipeline.get_element("PE_1")

    def check():
        pipeline._enable_thread_local("test", "pp")
        try:
            return (pe_1.get_parameter("pe_1_inc"), pe_1.get_parameter("p_3"), pe_1.get_parameter("p_2"),
                    pe_1.get_parameter("missing", default=5))
        finally:
            pipeline._disable_thread_local("test")
    a, b, c, d = event.call_on_loop(check)
    assert a == (7, True)               # stream "Element.name" wins
    assert b == ("stream", True)        # then element, then stream "name"
    assert c == (0, True)               # then pipeline definition
    assert d == (5, False)              # default, found=False
    pipeline.create_frame({"stream_id": "pp", "frame_id": 0}, {"b": 1})
    info, data = q.get(timeout=5)
    assert data["f"] == 2 * (1 + 7 + 1)


def test_process_frame_over_message_bus(aiko_process):
    """MQTT-style ingress: S-expression on the pipeline's /in topic, output on /out."""
    aiko = aiko_process
    pipeline, q = _create(DIAMOND, stream_id=None)
    outputs = queue.Queue()
    event.call_on_loop(lambda: aiko.process.add_message_handler(
        lambda _a, topic, payload: outputs.put(payload), pipeline.topic_out))
    aiko.aiko.message.publish(pipeline.topic_in, "(process_frame (stream_id: 9 frame_id: 3) (b: 0))")
    # stream 9 does not exist -> warn, no output; default stream "*" auto-creates
    aiko.aiko.message.publish(pipeline.topic_in, "(process_frame (stream_id: * frame_id: 4) (b: 1))")
    payload = outputs.get(timeout=5)
    from aiko_services_amd.utils.sexpr import parse
    cmd, (info, data) = parse(payload)
    assert cmd == "process_frame" and info["frame_id"] == "4" and data["f"] == "6"


@pytest.mark.parametrize("name", ["pipeline_local.json", "pipeline_paths.json", "pipeline_example.json"])
def test_reference_definitions_parse(name):
    d = parse_pipeline_definition(str(GOLDEN / name))
    assert d.elements


def test_reference_pipeline_local_runs(aiko_process, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)   # PE_Inspect writes z_inspect.txt in cwd
    path = GOLDEN / "pipeline_local.json"
    d = parse_pipeline_definition(str(path))
    pipeline, q = _create(d, stream_id="r1", pathname=str(path))
    pipeline.create_frame({"stream_id": "r1", "frame_id": 0}, {"b": 0})
    info, data = q.get(timeout=5)
    assert data["f"] == 4
    assert (tmp_path / "z_inspect.txt").exists()


def test_reference_text_pipeline_runs(aiko_process, tmp_path, monkeypatch):
    media = GOLDEN
    (tmp_path / "data_in").symlink_to(media / "data_in")
    (tmp_path / "data_out").mkdir()
    monkeypatch.chdir(tmp_path)
    d = parse_pipeline_definition(str(media / "text_pipeline_0.json"))
    pipeline, q = _create(d, stream_id="rt")
    outs = [q.get(timeout=10) for _ in range(3)]
    assert len(outs) == 3
    written = sorted((tmp_path / "data_out").glob("out_*.txt"))
    assert len(written) == 3
    assert written[0].read_text() == (media / "data_in" / "in_00.txt").read_text().title()


def test_trace_export_and_latency_stats(aiko_process, tmp_path):
    """Chrome-trace export of frame / element spans and p50 / p99 latency."""
    from aiko_services_amd.utils import trace
    tracer = trace.enable_tracing()
    try:
        pipeline, q = _create(dict(DIAMOND, name="p_traced"), stream_id="7")
        for i in range(4):
            pipeline.create_frame({"stream_id": "7", "frame_id": i}, {"b": i})
        for _ in range(4):
            q.get(timeout=5)
        path = tracer.export(str(tmp_path / "trace.json"))
    finally:
        trace.disable_tracing()
    evs = json.load(open(path))["traceEvents"]
    spans = [e for e in evs if e.get("ph") == "X"]
    frames = [e for e in spans if e["cat"] == "frame" and e["args"]["stream_id"] == "7"]
    elems = [e for e in spans if e["cat"] == "element" and e["args"]["stream_id"] == "7"]
    assert len(frames) == 4 and len(elems) == 4 * 5
    for f in frames:   # element spans nest inside their frame's span
        inner = [e for e in elems if e["args"]["frame_id"] == f["args"]["frame_id"]]
        assert all(f["ts"] - 1 <= e["ts"] and e["ts"] + e["dur"] <= f["ts"] + f["dur"] + 1 for e in inner)
    stats = pipeline.latency_stats()
    assert stats["frames"] >= 4 and 0 <= stats["p50_ms"] <= stats["p99_ms"] <= stats["max_ms"]
    summary = tracer.summary()
    assert summary["element:PE_1"]["count"] >= 4, summary


def test_fault_injection_element_error_and_message_drop(aiko_process):
    """Fault hooks: an injected element error takes the StreamEvent.ERROR path;
    control messages matching a topic filter are dropped reproducibly."""
    from aiko_services_amd.message import Loopback, LoopbackBus
    from aiko_services_amd.pipeline.stream import StreamState
    from aiko_services_amd.utils import fault
    plan = fault.inject("error=PE_2@2")
    try:
        pipeline, q = _create(dict(DIAMOND, name="p_fault"), stream_id="5")
        pipeline.create_frame({"stream_id": "5", "frame_id": 1}, {"b": 1})
        info, data = q.get(timeout=5)
        assert info["state"] == 0 and data["f"] == 6
        pipeline.create_frame({"stream_id": "5", "frame_id": 2}, {"b": 2})
        info, data = q.get(timeout=5)
        assert info["state"] == StreamState.ERROR and "injected fault" in data["diagnostic"]
        assert plan.frames_seen >= 2
    finally:
        fault.clear()
    bus = LoopbackBus()
    got = []
    rx = Loopback(message_handler=lambda c, u, m: got.append(m.topic), topics_subscribe=["t/#"], bus=bus)
    tx = Loopback(bus=bus)
    plan = fault.inject("drop=0.5@t/lossy", seed=3)
    try:
        for _ in range(200):
            tx.publish("t/lossy", "x")
            tx.publish("t/safe", "x")
    finally:
        fault.clear()
    assert got.count("t/safe") == 200
    assert got.count("t/lossy") == 200 - plan.dropped and 60 < plan.dropped < 140


EXAMPLES = Path(__file__).resolve().parents[1] / "aiko_services_amd/examples/pipeline/definitions"


def _load_example(name):
    return parse_pipeline_definition_dict(json.loads((EXAMPLES / name).read_text()), str(EXAMPLES / name))


def test_example_definitions_run(aiko_process):
    """The shipped example definitions (no reference checkout needed)."""
    import numpy as np
    p, q = _create(_load_example("diamond.json"), name="ex_diamond", stream_id="11")
    p.create_frame({"stream_id": "11", "frame_id": 0}, {"a": 1})
    info, data = q.get(timeout=5)
    assert info["state"] == 0 and data["f"] == 2 * (1 + 1 + 10 + 1)
    for head, expect in (("PE_IN", "x:in:text:out"), ("PE_IN_B", "x:in:out")):
        p, q = _create(_load_example("graph_paths.json"), name=f"ex_paths_{head}", stream_id="12",
                       graph_path=head)
        p.create_frame({"stream_id": "12", "frame_id": 0}, {"in_a": "x"})
        info, data = q.get(timeout=5)
        assert data["out_c"] == expect, (head, data)
    p, q = _create(_load_example("name_mapping.json"), name="ex_mapping", stream_id="13")
    outs = [q.get(timeout=10) for _ in range(5)]
    assert all(0 <= int(d["i"]) - 1 <= 9 for _, d in outs)
    p, q = _create(_load_example("codec.json"), name="ex_codec", stream_id="14")
    arr = np.arange(12, dtype=np.float32).reshape(3, 4)
    p.create_frame({"stream_id": "14", "frame_id": 0}, {"data": arr})
    info, data = q.get(timeout=5)
    assert np.array_equal(data["data"], arr)


def test_image_synthetic_source(aiko_process):
    M = "aiko_services_amd.elements.media.image_io"
    d = {"version": 0, "name": "p_synth", "runtime": "python", "graph": ["(ImageSynthetic ImageOutput)"],
         "parameters": {"width": 64, "height": 48, "batch": 2, "limit": 3},
         "elements": [{"name": "ImageSynthetic", "input": [{"name": "images", "type": "[image]"}], "output": [{"name": "images", "type": "[image]"}],
                       "deploy": {"local": {"module": M}}},
                      {"name": "ImageOutput", "input": [{"name": "images", "type": "[image]"}],
                       "output": [{"name": "images", "type": "[image]"}], "deploy": {"local": {"module": M}}}]}
    p, q = _create(d, name="p_synth", stream_id="21")
    outs = [q.get(timeout=10) for _ in range(3)]
    for info, data in outs:
        assert len(data["images"]) == 2 and data["images"][0].shape == (48, 64, 3)


def test_speech_example_elements(aiko_process, tmp_path):
    """examples/speech: WAV write -> LRU framing (reads + deletes the file); LLM element against
    a local OpenAI-compatible stub server."""
    import http.server
    import threading
    import numpy as np
    M = "aiko_services_amd.examples.speech.speech_elements"

    def el(name, ins, outs, params=None):
        return {"name": name, "input": [{"name": n, "type": "any"} for n in ins],
                "output": [{"name": n, "type": "any"} for n in outs], "parameters": params or {},
                "deploy": {"local": {"module": M}}}
    d = {"version": 0, "name": "p_speech", "runtime": "python", "graph": ["(PE_AudioWriteFile PE_AudioFraming)"],
         "elements": [el("PE_AudioWriteFile", ["audio"], ["audio"],
                         {"path_template": str(tmp_path / "chunk_{frame_id:03}.wav")}),
                      el("PE_AudioFraming", ["audio"], ["audio"], {"window_chunks": 2, "delete_input": True})]}
    p, q = _create(d, name="p_speech", stream_id="31")
    chunks = [np.full(1600, 0.1 * (i + 1), np.float32) for i in range(3)]
    for i, c in enumerate(chunks):
        p.create_frame({"stream_id": "31", "frame_id": i}, {"audio": c})
    outs = [q.get(timeout=5)[1]["audio"] for _ in range(3)]
    assert [len(o) for o in outs] == [1600, 3200, 3200]
    assert np.allclose(outs[2][:1600], 0.2, atol=1e-3) and np.allclose(outs[2][1600:], 0.3, atol=1e-3)
    assert not list(tmp_path.glob("*.wav"))                          # inputs deleted

    class Stub(http.server.BaseHTTPRequestHandler):
        def do_POST(self):
            body = json.loads(self.rfile.read(int(self.headers["Content-Length"])))
            reply = json.dumps({"choices": [{"message": {"content": body["messages"][0]["content"].upper()}}]})
            self.send_response(200)
            self.send_header("Content-Type", "application/json")
            self.end_headers()
            self.wfile.write(reply.encode())

        def log_message(self, *a):
            pass
    server = http.server.HTTPServer(("127.0.0.1", 0), Stub)
    threading.Thread(target=server.serve_forever, daemon=True).start()
    try:
        d = {"version": 0, "name": "p_llm", "runtime": "python", "graph": ["(PE_SpeechFraming PE_LLM)"],
             "elements": [el("PE_SpeechFraming", ["text"], ["text"]),
                          el("PE_LLM", ["text"], ["text"], {"url": f"http://127.0.0.1:{server.server_port}/v1"})]}
        p, q = _create(d, name="p_llm", stream_id="32")
        p.create_frame({"stream_id": "32", "frame_id": 0}, {"text": "aloha honua"})
        info, data = q.get(timeout=10)
        assert info["state"] == 0 and data["text"] == "ALOHA HONUA"
    finally:
        server.shutdown()


def test_llm_example_backends(aiko_process):
    """examples/llm PE_LLM: Ollama /api/chat (default llm_type) and OpenAI chat-completions
    against a local stub; the system prompt carries the robot vocabulary and the objects
    published on {namespace}/detections within the last second; <silence> passes through; a
    dead server ends the frame with an error; PE_COQUI_TTS passes text through."""
    import http.server
    import threading
    from aiko_services_amd.examples.llm import elements_llm as L
    seen = []

    class Stub(http.server.BaseHTTPRequestHandler):
        def do_POST(self):
            body = json.loads(self.rfile.read(int(self.headers["Content-Length"])))
            seen.append((self.path, body))
            text = "(action " + body["messages"][1]["content"].split()[-1] + ")"
            reply = ({"message": {"role": "assistant", "content": text}} if self.path == "/api/chat"
                     else {"choices": [{"message": {"content": text}}]})
            data = json.dumps(reply).encode()
            self.send_response(200)
            self.send_header("Content-Type", "application/json")
            self.send_header("Content-Length", str(len(data)))
            self.end_headers()
            self.wfile.write(data)

        def log_message(self, *a):
            pass
    server = http.server.HTTPServer(("127.0.0.1", 0), Stub)
    threading.Thread(target=server.serve_forever, daemon=True).start()
    M = "aiko_services_amd.examples.llm.elements_llm"

    def el(name, params=None):
        return {"name": name, "input": [{"name": "text", "type": "str"}], "output": [{"name": "text", "type": "str"}],
                "parameters": params or {}, "deploy": {"local": {"module": M}}}
    try:
        base = f"http://127.0.0.1:{server.server_port}"
        d = {"version": 0, "name": "p_llm_ollama", "runtime": "python", "graph": ["(PE_LLM PE_COQUI_TTS)"],
             "elements": [el("PE_LLM", {"url": base}), el("PE_COQUI_TTS")]}
        p, q = _create(d, name="p_llm_ollama", stream_id="61")
        aiko_process.aiko.message.publish(L.topic_detections(), "(detections person ball)")
        time.sleep(0.2)
        p.create_frame({"stream_id": "61", "frame_id": 0}, {"text": "please sit"})
        info, data = q.get(timeout=10)
        assert info["state"] == 0 and data["text"] == "(action sit)"
        path, body = seen[-1]
        assert path == "/api/chat" and body["stream"] is False and body["model"] == L.LLM_MODEL_NAME
        assert body["options"]["temperature"] == 0.0
        assert "(action wag)" in body["messages"][0]["content"] and "person ball" in body["messages"][0]["content"]
        n = len(seen)
        p.create_frame({"stream_id": "61", "frame_id": 1}, {"text": "<silence>"})
        info, data = q.get(timeout=10)
        assert data["text"] == "<silence>" and len(seen) == n
        d = {"version": 0, "name": "p_llm_openai", "runtime": "python", "graph": ["(PE_LLM)"],
             "elements": [el("PE_LLM", {"llm_type": "openai", "url": base + "/v1", "model": "m"})]}
        p, q = _create(d, name="p_llm_openai", stream_id="62")
        p.create_frame({"stream_id": "62", "frame_id": 0}, {"text": "turn left"})
        info, data = q.get(timeout=10)
        assert data["text"] == "(action left)" and seen[-1][0] == "/v1/chat/completions"
    finally:
        server.shutdown()
        server.server_close()
    d = {"version": 0, "name": "p_llm_down", "runtime": "python", "graph": ["(PE_LLM)"],
         "elements": [el("PE_LLM", {"url": base, "timeout": 2})]}
    p, q = _create(d, name="p_llm_down", stream_id="63")
    p.create_frame({"stream_id": "63", "frame_id": 0}, {"text": "sit"})
    info, data = q.get(timeout=10)
    assert info["state"] != 0


def test_audio_spectrum_and_remote_elements(aiko_process):
    """Reference dead audio elements: FFT -> filter -> bands -> XY graph; array frames sent by
    PE_RemoteSend0 over a binary topic arrive as new frames of PE_RemoteReceive0's pipeline."""
    import numpy as np
    M = "aiko_services_amd.elements.media.audio_io"

    def el(name, ins, outs, params=None):
        return {"name": name, "input": [{"name": n, "type": "any"} for n in ins],
                "output": [{"name": n, "type": "any"} for n in outs], "parameters": params or {},
                "deploy": {"local": {"module": M}}}
    d = {"version": 0, "name": "p_spectrum", "runtime": "python",
         "graph": ["(PE_FFT PE_AudioFilter PE_AudioResampler PE_GraphXY)"],
         "elements": [el("PE_FFT", ["audio_samples"], ["amplitudes", "frequencies"]),
                      el("PE_AudioFilter", ["amplitudes", "frequencies"], ["amplitudes", "frequencies"],
                         {"amplitude_minimum": 10, "amplitude_maximum": 1e9}),
                      el("PE_AudioResampler", ["amplitudes", "frequencies"], ["amplitudes", "frequencies"],
                         {"band_count": 4, "frequency_maximum": 4000}),
                      el("PE_GraphXY", ["amplitudes", "frequencies"], ["amplitudes", "frequencies", "image"],
                         {"width": 64, "height": 48, "frequency_maximum": 4000, "amplitude_maximum": 0})]}
    p, q = _create(d, name="p_spectrum", stream_id="41")
    t = np.arange(16000) / 16000.0
    x = (np.sin(2 * np.pi * 440 * t) + 0.5 * np.sin(2 * np.pi * 2500 * t)).astype(np.float32)
    p.create_frame({"stream_id": "41", "frame_id": 0}, {"audio_samples": x})
    info, out = q.get(timeout=5)
    assert info["state"] == 0 and out["image"].shape == (48, 64, 3) and out["image"].any()
    assert len(out["amplitudes"]) == 4
    assert np.argmax(out["amplitudes"]) == 0 and out["amplitudes"][2] > 0   # 440 Hz band, 2.5 kHz band

    rx = {"version": 0, "name": "p_rx", "runtime": "python", "graph": ["(PE_RemoteReceive0)"],
          "elements": [el("PE_RemoteReceive0", ["audio"], ["audio"], {"stream_id": "0"})]}
    tx = {"version": 0, "name": "p_tx", "runtime": "python", "graph": ["(PE_RemoteSend0)"],
          "elements": [el("PE_RemoteSend0", ["audio"], [])]}
    _, qr = _create(rx, name="p_rx", stream_id="0")
    ptx, qt = _create(tx, name="p_tx", stream_id="42")
    for i in range(2):
        ptx.create_frame({"stream_id": "42", "frame_id": i}, {"audio": np.full(8, i, np.int16)})
    got = [qr.get(timeout=5)[1]["audio"] for _ in range(2)]
    assert [g.tolist() for g in got] == [[0] * 8, [1] * 8]
    from aiko_services_amd.elements.media.audio_io import PE_MicrophoneSD, decode_array, encode_array
    assert decode_array(encode_array(np.array(["hi"]))).tolist() == ["hi"]
    with pytest.raises(Exception):
        _create({"version": 0, "name": "p_mic", "runtime": "python", "graph": ["(PE_MicrophoneSD)"],
                 "elements": [el("PE_MicrophoneSD", [], ["audio"])]}, name="p_mic", stream_id="43")
    assert PE_MicrophoneSD.BACKEND == "sounddevice"


def test_aruco_example_fallback_detector(aiko_process):
    """examples/aruco_marker: numpy fallback finds two markers (one turned 90 degrees) with
    rotation-invariant ids and marker-frame corners; the overlay draws on the image."""
    import numpy as np
    from aiko_services_amd.examples.aruco_marker.aruco import make_marker
    a, b = make_marker(0b1000_0110_0010_1101, 6), make_marker(0b0001_0000_0111_0011, 5)
    img = np.full((120, 160, 3), 255, np.uint8)
    img[10:10 + a.shape[0], 10:10 + a.shape[1]] = a[..., None]
    rb = np.rot90(b, -1)                                    # turned 90 degrees clockwise
    img[50:50 + rb.shape[0], 90:90 + rb.shape[1]] = rb[..., None]
    M = "aiko_services_amd.examples.aruco_marker.aruco"
    d = {"version": 0, "name": "p_aruco", "runtime": "python",
         "graph": ["(ArucoMarkerDetector ArucoMarkerOverlay)"],
         "elements": [{"name": "ArucoMarkerDetector", "input": [{"name": "images", "type": "[image]"}],
                       "output": [{"name": "overlays", "type": "[overlay]"}], "deploy": {"local": {"module": M}}},
                      {"name": "ArucoMarkerOverlay", "input": [{"name": "images", "type": "[image]"},
                                                                {"name": "overlays", "type": "[overlay]"}],
                       "output": [{"name": "images", "type": "[image]"}, {"name": "overlays", "type": "[overlay]"}],
                       "deploy": {"local": {"module": M}}}]}
    p, q = _create(d, name="p_aruco", stream_id="51")
    p.create_frame({"stream_id": "51", "frame_id": 0}, {"images": [img]})
    info, out = q.get(timeout=5)
    assert info["state"] == 0
    ov = out["overlays"][0]
    ids = sorted(int(i) for i in ov["ids"].reshape(-1))
    from aiko_services_amd.examples.aruco_marker.aruco import _code, GRID
    def canon(code):
        bits = np.array([(code >> i) & 1 for i in range(16)]).reshape(4, 4)
        return min(_code(np.rot90(bits, -k)) for k in range(4))
    assert ids == sorted([canon(0b1000_0110_0010_1101), canon(0b0001_0000_0111_0011)])
    assert len(ov["corners"]) == 2 and ov["corners"][0].shape == (1, 4, 2)
    assert (out["images"][0] != img).any()


def test_aruco_original_dictionary_ids(aiko_process):
    """aruco_tags DICT_ARUCO_ORIGINAL: the fallback decodes the original-ArUco ids (2 bits per
    codeword row) in every rotation, with the marker's own top-left corner first; a grid whose
    rows are not codewords is rejected."""
    import numpy as np
    from aiko_services_amd.examples.aruco_marker.aruco import decode_original, make_marker_original, original_bits
    assert all(decode_original(original_bits(i)) == i for i in range(1024))
    bad = original_bits(5).copy()
    bad[2, 0] ^= 1                                          # row 2 no longer a codeword
    assert decode_original(bad) is None
    img = np.full((160, 240, 3), 255, np.uint8)
    placed = {}
    for n, (mid, k, y, x) in enumerate([(213, 0, 8, 8), (517, 1, 8, 120), (42, 2, 90, 8), (999, 3, 90, 120)]):
        m = np.rot90(make_marker_original(mid, 6), k)       # k quarter turns counter-clockwise
        img[y:y + m.shape[0], x:x + m.shape[1]] = m[..., None]
        side = m.shape[0] - 12                              # marker without its quiet zone
        tl = [(x + 6, y + 6), (x + 6, y + 6 + side), (x + 6 + side, y + 6 + side), (x + 6 + side, y + 6)][k]
        placed[mid] = tl
    M = "aiko_services_amd.examples.aruco_marker.aruco"
    d = {"version": 0, "name": "p_aruco_orig", "runtime": "python", "graph": ["(ArucoMarkerDetector)"],
         "elements": [{"name": "ArucoMarkerDetector", "parameters": {"aruco_tags": "DICT_ARUCO_ORIGINAL"},
                       "input": [{"name": "images", "type": "[image]"}],
                       "output": [{"name": "overlays", "type": "[overlay]"}], "deploy": {"local": {"module": M}}}]}
    p, q = _create(d, name="p_aruco_orig", stream_id="52")
    p.create_frame({"stream_id": "52", "frame_id": 0}, {"images": [img]})
    info, out = q.get(timeout=5)
    ov = out["overlays"][0]
    got = {int(i): tuple(c.reshape(4, 2)[0]) for i, c in zip(ov["ids"].reshape(-1), ov["corners"])}
    assert sorted(got) == sorted(placed)
    for mid, tl in placed.items():
        assert got[mid] == tl, (mid, got[mid], tl)


def test_destroy_stream_returns_admission_credits(aiko_process):
    """the admission window is shared by the whole pipeline, so a stream
    destroyed with frames in flight (or with admitted frames that never came to exist) must
    return every credit, or later streams starve at admit_frame."""
    from aiko_services_amd.pipeline.stream import Frame
    d = json.loads(json.dumps(DIAMOND))
    d["parameters"]["frame_window"] = 2
    pipeline, q = _create(d, stream_id="w1")
    assert pipeline.frame_window() == 2
    released = []
    # two frames in flight on stream w1: admitted and present in the stream, never completed
    for fid in (0, 1):
        assert pipeline.admit_frame("w1", fid, timeout=0)
        frame = Frame()
        frame.on_complete.append(lambda fid=fid: released.append(fid))
        pipeline.stream_leases["w1"].stream.frames[fid] = frame
    assert not pipeline.admit_frame("w2", 0, timeout=0)           # window full
    event.call_on_loop(lambda: pipeline.destroy_stream("w1"))
    assert sorted(released) == [0, 1]                              # their slots came back
    assert pipeline.admit_frame("w2", 0, timeout=0)                # and so did the credits
    # a frame admitted for a stream that no longer exists is rejected AND un-admitted
    assert pipeline.admit_frame("gone", 7, timeout=0)
    event.call_on_loop(lambda: pipeline.process_frame({"stream_id": "gone", "frame_id": 7}, {"b": 1}))
    assert ("gone", 7) not in pipeline._admitted
    # credits held by a stream whose frames never reached the engine go with the stream
    pipeline._admit_release(("w2", 0))
    assert pipeline.admit_frame("w3", 0, timeout=0) and pipeline.admit_frame("w3", 1, timeout=0)
    event.call_on_loop(lambda: pipeline.create_stream("w3"))
    event.call_on_loop(lambda: pipeline.destroy_stream("w3"))
    assert not any(k[0] == "w3" for k in pipeline._admitted)


def test_destroy_stream_keeps_credit_of_stuck_zero_copy_send(aiko_process, monkeypatch):
    """a destroyed stream's frame whose zero-copy send is still in flight
    (a Dropped handle owns its FramePool slot) keeps its admission credit until the transfer
    completes; the bulk release of the stream must not hand that credit out early."""
    from aiko_services_amd.pipeline.stream import Frame
    d = json.loads(json.dumps(DIAMOND))
    d["parameters"]["frame_window"] = 1
    pipeline, q = _create(d, stream_id="z1")
    monkeypatch.setattr(pipeline, "_watch_hops", lambda: None)

    class StuckSend:                       # stands in for parallel.hop.Dropped
        def __init__(self):
            self.callbacks = []

        def then(self, fn):
            self.callbacks.append(fn)

        def complete(self):
            for fn in self.callbacks:
                fn()

    slot_back = []
    assert pipeline.admit_frame("z1", 0, timeout=0)
    frame = Frame()
    frame.on_complete.append(lambda: slot_back.append(0))
    lease = pipeline.stream_leases["z1"]
    lease.stream.frames[0] = frame
    stuck = StuckSend()

    def destroy():
        pipeline._release_frame(lease.stream, 0, after=stuck)      # destroy_stream's drop path
        pipeline._admit_release_stream("z1")
    event.call_on_loop(destroy)
    assert slot_back == []                                          # slot still read by the send
    assert not pipeline.admit_frame("z2", 0, timeout=0.2)            # ... and its credit held
    stuck.complete()                                                 # poll_dropped: transfer done
    assert slot_back == [0]
    assert pipeline.admit_frame("z2", 0, timeout=0)


def test_dict_swag_never_enters_hop_decode(aiko_process, monkeypatch):
    """with a hop data plane up, reference-style frames whose swag holds
    plain nested dicts (no tensor tokens, no encoded DeviceResult, no hop_rank) are never
    handed to ``HopPlane.decode`` — only messages that went through ``HopPlane.encode`` are."""
    from aiko_services_amd.parallel import hop, hop_state
    assert not hop_state.needs_decode({"stream_id": "1", "frame_id": 0}, {"b": {"x": 1, "y": [1, 2]}})
    assert not hop_state.needs_decode({}, {"s": "T not a token", "m": {"k": "v"}})
    assert hop_state.needs_decode({"hop_rank": 0}, {})
    assert hop_state.needs_decode({}, {"x": "T@0/0/0/float32/2x3"})
    assert hop_state.needs_decode({}, {"r": {hop_state.RESULT_KEY: "1"}})
    plane = hop.init_plane([(0, 0)], device="cpu", depth=2)
    calls = []

    def boom(*a, **k):
        calls.append(a)
        raise AssertionError("hop.decode called for a plain reference frame")
    monkeypatch.setattr(hop.HopPlane, "decode", boom)
    monkeypatch.setattr(hop.HopPlane, "decode_async", boom)
    try:
        pipeline, q = _create(DIAMOND, stream_id="sw")
        pipeline.create_frame({"stream_id": "sw", "frame_id": 0}, {"b": 2, "meta": {"camera": {"id": 3}}})
        info, data = q.get(timeout=5)
        assert info["state"] == 0 and "f" in data and not calls
    finally:
        hop.shutdown_plane()
    assert hop_state.plane() is None
