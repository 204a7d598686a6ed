from vstyler.models import FaceAdapter, FaceBlock, FaceEncoder, WanAnimateAdapter  # noqa: F401
