"""Cases shared by the downscale tests: the size table worked out from the reference's text in
numpy f32, and the axis sizes whose filter tables the library reproduces bit for bit."""
import resize_model as rm

# (in_w, in_h, mode, size) -> (out_w, out_h): OpenStreams' rule (video_reader_unit.cpp:155-206)
SIZE_TABLE = [
    (3840, 2160, rm.TO_MIN_SIZE, 360, 640, 360),
    (1920, 1080, rm.TO_MIN_SIZE, 360, 640, 360),
    (1280, 720, rm.TO_MIN_SIZE, 360, 640, 360),
    (2160, 3840, rm.TO_MIN_SIZE, 360, 360, 640),
    (720, 480, rm.TO_MIN_SIZE, 360, 542, 361),     # the f32 factor is 0.75000006
    (1000, 700, rm.TO_MIN_SIZE, 360, 516, 360),    # f64 arithmetic would give 515 before evening
    (272, 480, rm.TO_MIN_SIZE, 360, 272, 480),     # capped to factor 1
    (97, 61, rm.TO_MIN_SIZE, 360, 98, 61),         # factor 1, width forced even
    (1280, 720, rm.TO_MIN_SIZE, 48, 86, 49),
    (97, 61, rm.TO_MIN_SIZE, 48, 78, 48),
    (130, 70, rm.TO_MIN_SIZE, 48, 90, 48),
    (130, 70, rm.TO_MAX_SIZE, 48, 48, 26),
    (96, 72, rm.TO_MIN_SIZE, 48, 64, 48),
    (96, 72, rm.TO_MAX_SIZE, 48, 48, 36),
    (272, 480, rm.TO_MAX_SIZE, 48, 28, 49),
]

# (n_in, n_out) whose tables the library has to reproduce bit for bit (tests/test_capi_resize.py)
FILTER_CASES = [(3840, 640), (2160, 360), (97, 98), (97, 78), (96, 64), (96, 48), (70, 26), (61, 48),
                (768, 64), (5, 2), (2, 2), (1, 1)]
