from .models import Darknet, parse_config, yolov3_blocks  # noqa: F401
